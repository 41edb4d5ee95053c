"""Results of finished episodes, collected on the device while the batch keeps running.

With ``step(..., auto_reset=True)`` an env's counters, captures and step count are zeroed by the step after its episode ends, so
its result has to be taken in between.  ``EpisodeHarvest`` owns a small table of 64-bit accumulators, one row per caller-defined
GROUP of envs (one pairing of a tournament, one opponent of a league, or group 0 for the whole batch), and ``update()`` — one
kernel launch, ``ctf_harvest_episodes`` — adds the envs whose episode ended in the most recent step::

    h = EpisodeHarvest(vec, n_groups, groups)
    for _ in range(steps):
        vec.step_observe(actions, auto_reset=True)
        h.update()                      # once after EVERY step: twice counts twice, skipping a step loses the envs that reset
    print(h.results(0), h.metrics(0))

``results`` is the batched form of ``utils.duel(..., return_result=True)`` (reference utils.py:562-569), ``metrics`` of the
``env.metrics`` entries ``MetricsLogger.harvest_metrics`` reads (metrics_logger.py:137-159) — both as SUMS over the group's
harvested episodes: divide by ``episodes`` or pass a scaling factor.

The visitation maps (``metrics['agent_visitation_maps']``, what the reference's ``utils.plot_heatmaps`` sums over its duels) are
harvested too when asked for: ``EpisodeHarvest(vec, n_groups, groups, visitation=True)`` owns a second table, ``vis_acc`` int64
[n_groups, N, G, G], ``update()`` then issues a second launch (``ctf_harvest_visitation``) with the same arguments, which takes
exactly the same envs, and ``visitation(g)`` gives the group's maps as TRUE counts summed over its episodes (the reference's
uint8 maps are these ``& 0xFF``).  Across GPUs the table is small: ``all_reduce(h.vis_acc)`` is the whole reduction.
"""
import numpy as np

try:
    from . import _abi
    from .gridworld_ctf import metrics_from_counters
except ImportError:  # pragma: no cover
    import _abi
    from gridworld_ctf import metrics_from_counters

# words of a row (include/ctf_env.h, ctf_harvest_episodes)
EPISODES, WINS, DRAWS, LOSSES, CAPTURES_0, CAPTURES_1, STEPS = range(7)


class EpisodeHarvest:
    def __init__(self, vec, n_groups=1, groups=None, visitation=False):
        """vec: VecGridworldCtf.  groups: the group of every env (int tensor / array [E], values in [0, n_groups)), None =
        every env is group 0.  visitation: also harvest the visitation maps, into ``vis_acc`` int64 [n_groups, N, G, G]."""
        import torch

        self.vec = vec
        self.n_groups = int(n_groups)
        if self.n_groups < 1:
            raise ValueError("n_groups must be >= 1")
        self.H = int(vec.harvest_words)
        if self.H != _abi.HARVEST_HEAD + _abi.N_METRICS * vec.N_AGENTS:
            raise ValueError("harvest_words does not match the row layout of this binding")
        self.acc = torch.zeros((self.n_groups, self.H), dtype=torch.int64, device=vec.device)
        self.groups = None
        if groups is not None:
            g = groups if isinstance(groups, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(groups))
            if g.dim() != 1 or g.numel() != vec.n_envs or g.dtype.is_floating_point or g.dtype == torch.bool:
                raise ValueError(f"groups: expected {vec.n_envs} integer group ids")
            if g.numel() and (int(g.min()) < 0 or int(g.max()) >= self.n_groups):
                raise ValueError(f"groups: an id is outside [0, {self.n_groups})")
            self.groups = g.to(device=vec.device, dtype=torch.int32).contiguous()
        self.vis_acc = None
        if visitation:
            n, gsz = int(vec.N_AGENTS), int(vec.GRID_SIZE)
            if int(vec.visitation_words) != n * gsz * gsz:
                raise ValueError("visitation_words does not match N * G * G of this binding")
            self.vis_acc = torch.zeros((self.n_groups, n, gsz, gsz), dtype=torch.int64, device=vec.device)

    def update(self, mask=None, all_envs=False):
        """Add the envs whose episode ended in the most recent step (``all_envs``: every env as it stands — the cut of a
        truncated duel); ``mask`` uint8 [E]: only envs whose byte is non-zero.  One launch, stream-ordered (with
        ``visitation=True`` a second one, with the same arguments: the same envs)."""
        self.vec.harvest(self.acc, groups=self.groups, mask=mask, all_envs=all_envs)
        if self.vis_acc is not None:
            self.vec.harvest_visitation(self.vis_acc, groups=self.groups, mask=mask, all_envs=all_envs)

    def zero(self):
        self.acc.zero_()
        if self.vis_acc is not None:
            self.vis_acc.zero_()

    def table(self):
        """-> int64 numpy [n_groups, H]: one device-to-host copy."""
        return self.acc.cpu().numpy()

    def visitation_table(self):
        """-> int64 numpy [n_groups, N, G, G]: one device-to-host copy (``visitation=True`` only)."""
        if self.vis_acc is None:
            raise ValueError("this harvest was built without visitation=True")
        return self.vis_acc.cpu().numpy()

    def visitation(self, g, table=None):
        """-> {agent: int64 [G, G]}: the shape of the reference's ``metrics['agent_visitation_maps']``, summed over group g's
        harvested episodes WITHOUT the reference's uint8 wrap (``& 0xFF`` gives its maps)::

            m = h.metrics(g); m["agent_visitation_maps"] = h.visitation(g)

        ``table``: a copy taken earlier with ``visitation_table()``."""
        maps = np.asarray((self.visitation_table() if table is None else table)[g])
        return {i: maps[i].astype(np.int64) for i in range(maps.shape[0])}

    def results(self, g, table=None):
        """-> dict(episodes, wins, draws, losses (team 0's point of view), team_flag_captures {team: sum}, mean_steps) of group g.
        ``table``: a copy taken earlier with ``table()`` (several groups, one copy)."""
        row = (self.table() if table is None else table)[g]
        n = int(row[EPISODES])
        return dict(episodes=n, wins=int(row[WINS]), draws=int(row[DRAWS]), losses=int(row[LOSSES]),
                    team_flag_captures={0: int(row[CAPTURES_0]), 1: int(row[CAPTURES_1])},
                    mean_steps=int(row[STEPS]) / n if n else 0.0)

    def metrics(self, g, table=None):
        """-> the reference's metrics dict of group g without the visitation maps, every entry summed over the group's
        harvested episodes: what ``MetricsLogger.harvest_metrics(metrics, ..., scaling_factor)`` takes."""
        row = (self.table() if table is None else table)[g]
        n = self.vec.N_AGENTS
        counters = np.asarray(row[_abi.HARVEST_HEAD:]).reshape(_abi.N_METRICS, n)
        return metrics_from_counters(counters, (row[CAPTURES_0], row[CAPTURES_1]), self.vec.AGENT_TEAMS, self.vec.AGENT_TYPES, n)
