"""Recording the readable state of a few envs step by step, on the device, and turning the recording into the viewer record.

``StateRecorder`` owns device buffers ``[capacity][n16][...]`` for a fixed list of envs; ``record()`` is ONE
``VecGridworldCtf.get_states`` launch (``ctf_export_states``, include/ctf_env.h) into the next frame — stream-ordered, no
synchronisation, no ``get_state`` round trip per env — and ``frames()`` brings everything recorded so far to the host with one
transfer per field.  ``frames_to_trajectory`` builds from such frames the dict ``utils.duel_json`` (reference utils.py:728-815)
writes for one env: what ``duel.duel_trajectory`` builds from one ``get_state`` per step.
"""
import numpy as np

__all__ = ["StateRecorder", "frames_to_trajectory"]

DEFAULT_FIELDS = ("grid", "pos", "has_flag", "team_captures")
_PAD = 16  # records per frame are padded to a multiple of this: every frame's slice of every array stays 16-byte aligned


class StateRecorder:
    """``idx``: the envs to record (host sequence or tensor; repeats allowed).  ``capacity``: frames the buffers hold.  ``fields``:
    names of ``get_states`` fields.  The index list is padded to a multiple of 16 by repeating its last entry, so that frame t of
    every array starts on a 16-byte boundary whatever N and G are; ``frames()`` trims the padding."""

    def __init__(self, vec, idx, capacity, fields=DEFAULT_FIELDS):
        import torch

        host = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx)
        if host.ndim != 1 or host.size < 1 or not np.issubdtype(host.dtype, np.integer):
            raise ValueError("StateRecorder: expected a non-empty 1-D integer index list")
        if int(host.min()) < 0 or int(host.max()) >= vec.n_envs:
            raise ValueError(f"StateRecorder: an index is outside [0, {vec.n_envs})")
        if int(capacity) < 1:
            raise ValueError("StateRecorder: capacity must be at least 1")
        specs = vec._state_specs()
        self.fields = tuple(fields)
        for f in self.fields:
            if f not in specs or f == "visitation":
                raise ValueError(f"StateRecorder: unknown field {f!r}")
        self.vec, self.n, self.capacity, self.t = vec, int(host.size), int(capacity), 0
        self.n16 = (self.n + _PAD - 1) // _PAD * _PAD
        padded = np.concatenate([host, np.full(self.n16 - self.n, host[-1], host.dtype)]).astype(np.int32)
        self.idx = torch.from_numpy(padded).to(vec.device)
        self.buf = {f: torch.zeros((self.capacity, self.n16) + tuple(specs[f][1]), dtype=specs[f][0], device=vec.device) for f in self.fields}
        self._views = [None] * self.capacity  # frame t's slices, made once

    def record(self):
        """Frame t := the envs' state now (one stream-ordered launch); raises IndexError when the buffers are full."""
        if self.t >= self.capacity:
            raise IndexError(f"StateRecorder: all {self.capacity} frames are taken")
        if self._views[self.t] is None:
            self._views[self.t] = {f: b[self.t] for f, b in self.buf.items()}
        self.vec.get_states(idx=self.idx, fields=self.fields, out=self._views[self.t])
        self.t += 1

    def reset(self):
        """Forget the recorded frames (the buffers are reused)."""
        self.t = 0

    def frames(self):
        """-> dict name -> numpy array [t, n, ...] of the t frames recorded so far: one device-to-host transfer per field."""
        return {f: b[:self.t].cpu().numpy()[:, :self.n] for f, b in self.buf.items()}


def _tiles_of(grid):
    return [{"x": int(x), "z": int(z), "type": 0} for z, x in zip(*np.where(grid == 2))] + \
           [{"x": int(x), "z": int(z), "type": 1} for z, x in zip(*np.where(grid == 3))]


def frames_to_trajectory(vec_static, frames, k):
    """The ``utils.duel_json`` dict of recorded env ``k`` from ``frames`` (``StateRecorder.frames()`` with at least grid, pos,
    has_flag and team_captures): frame 0 is the state after ``reset()``, frame s the state after step s.  ``vec_static`` supplies
    what does not change (``N_AGENTS``, ``GRID_SIZE``, ``AGENT_TEAMS``, ``AGENT_TYPES``, ``derived['kwargs']['SCENARIO']``); no
    device is touched.  Same keys, orders and plain ints as ``duel.duel_trajectory``."""
    n, g = vec_static.N_AGENTS, vec_static.GRID_SIZE
    scen = vec_static.derived["kwargs"]["SCENARIO"]
    grids, poss, flags, caps = (np.asarray(frames[f])[:, k] for f in ("grid", "pos", "has_flag", "team_captures"))
    grid0 = grids[0].reshape(g, g)
    out = {
        "grid_size": g,
        "flag_pos": {f"{t}": {"x": v[1], "z": v[0]} for t, v in scen["FLAG_POSITIONS"].items()},
        "spawn_pos": {f"{t}": {"x": v[1], "z": v[0]} for t, v in scen["SPAWN_POSITIONS"].items()},
        "agent_config": [{"team": vec_static.AGENT_TEAMS[i], "type": vec_static.AGENT_TYPES[i],
                          "start_x": scen["AGENT_STARTING_POSITIONS"][i][1], "start_z": scen["AGENT_STARTING_POSITIONS"][i][0]} for i in range(n)],
        "block_tiles": [{"x": int(x), "z": int(z)} for z, x in zip(*np.where(grid0 == 1))],
        "destructible_tiles": _tiles_of(grid0),
    }
    movement, tiles, scores = [], [], []
    for s in range(1, grids.shape[0]):
        movement.append([{"x": int(poss[s, i, 1]) - int(poss[s - 1, i, 1]), "z": int(poss[s, i, 0]) - int(poss[s - 1, i, 0]),
                          "has_flag": int(flags[s, i])} for i in range(n)])
        tiles.append(_tiles_of(grids[s].reshape(g, g)))
        scores.append([{"t0": int(caps[s, 0]), "t1": int(caps[s, 1])}])
    out["movement"], out["tiles"], out["scores"] = movement, tiles, scores
    return out
