"""Batched duel: the counterpart of ``utils.duel`` (reference utils.py:500-573) for E envs at once.

Per env it reproduces the reference loop: ``reset()``; every step each agent observes (team 0 raw, team 1 flipped),
team-0 agents are driven by ``agent`` and team-1 agents by ``opponent`` whose actions are mapped back through
``REVERSED_ACTION_MAP`` (utils.py:535-551); the loop ends when the env reports ``done`` or after ``max_steps + 1``
steps (``step_count > max_steps``, utils.py:559).  All envs of a batch share GAME_STEPS and start together, so they
all stop at the same step.  Returns what the reference returns per env: the result sign (utils.py:562-569) and the
counters ``env.metrics`` holds (as tensors; ``VecGridworldCtf.counters``) and, with ``visitation=True``, its visitation maps
(``metrics['agent_visitation_maps']``, what ``utils.plot_heatmaps`` sums over its duels; utils.py:263-400) as true counts.
"""
import numpy as np

try:
    from .frames import StateRecorder, frames_to_trajectory
    from .harvest import EpisodeHarvest
    from .rollout import BatchedRolloutCollector
    from .scripted import ScriptedPolicy
except ImportError:  # pragma: no cover
    from scripted import ScriptedPolicy
    from frames import StateRecorder, frames_to_trajectory
    from harvest import EpisodeHarvest
    from rollout import BatchedRolloutCollector


def batched_duel(vec, agent, opponent, max_steps=256, visitation=False):
    """-> dict(result int8 [E] (+1 team 0 wins, 0 draw, -1 team 1 wins), team_flag_captures int32 [E, 2],
    metrics int32 [E, 13, N], steps int).  ``visitation=True`` adds ``visitation``, uint32 [E, N, G, G]: every env's maps at the
    end of its duel as true counts (one ``VecGridworldCtf.visitation`` launch).  ``(sum over envs) & 0xFF`` as uint8 is what
    ``utils.plot_heatmaps`` returns for the same duels: its ``+=`` on uint8 arrays wraps, and the sum of wrapped counts is
    congruent mod 256 to the wrapped sum of true counts."""
    import torch

    col = BatchedRolloutCollector(vec, 1, 0)  # reuses the policy plumbing; its rollout buffers hold one step
    use_codes = col.use_codes(agent, opponent)  # policies with a compact-observation path (policy_native.py) get the code bytes
    game_steps = int(vec.cfg.game_steps)
    n_steps = min(game_steps, int(max_steps) + 1)
    vec.reset()
    with torch.no_grad():
        for _ in range(n_steps):
            vec.step(col.joint_actions(agent, opponent, use_codes)[1])
    metrics, caps, _ = vec.counters()
    result = torch.sign(caps[:, 0] - caps[:, 1]).to(torch.int8)
    out = dict(result=result, team_flag_captures=caps, metrics=metrics, steps=n_steps)
    if visitation:
        out["visitation"] = vec.visitation()
    return out


def batched_tournament(vec, agents, opponents, max_steps=256, visitation=False, record=None):
    """Every pairing of ``agents`` (team 0) with ``opponents`` (team 1) in ONE batch: the batched form of the league's pairing
    loops (reference league_training.py:573-648).  The E envs are cut into ``len(agents) * len(opponents)`` contiguous, equal
    blocks, agent-major: block (a, b) — group ``a * len(opponents) + b`` — plays ``agents[a]`` against ``opponents[b]``, each env
    one duel as ``batched_duel`` plays it.  Every policy is called once per step, through ``get_action_and_value(grid, metadata,
    mask)``, on the rows of the envs it plays in.  One harvest after the last step gives the table.
    -> dict(episodes int64 [A, B], result_counts int64 [A, B, 3] (team 0 wins, draws, team 1 wins), win_rate float64 [A, B]
    (team 0's), table int64 [A * B, H] (``harvest.EpisodeHarvest``: ``results(g, table)`` / ``metrics(g, table)``), steps).  ``visitation=True`` adds ``visitation``,
    int64 numpy [A, B, N, G, G]: each pairing's visitation maps summed over its envs, true counts, from one
    ``harvest_visitation(all_envs=True)`` beside the harvest.  ``record=k`` records the first k envs of every pairing's block (one
    ``frames.StateRecorder`` launch per step) and adds ``trajectories``, [A][B][k] dicts as ``duel_trajectory`` builds them; the
    default makes no recorder, no key and no launch.  Any entry of ``opponents`` may be a ``scripted.ScriptedPolicy``: it decides once per
    step for the whole batch (one launch, no policy kernel) and its ENV actions reach ``step`` unmapped, in the rows of the envs it plays in."""
    import torch

    A, B, E = len(agents), len(opponents), vec.n_envs
    if A < 1 or B < 1 or E % (A * B):
        raise ValueError(f"{E} envs do not divide into {A} x {B} equal blocks")
    per = E // (A * B)
    col = BatchedRolloutCollector(vec, 1, 0)  # the policy plumbing of batched_duel
    dev = vec.device
    env = torch.arange(E, device=dev)
    harvest = EpisodeHarvest(vec, A * B, env // per, visitation=True) if visitation else EpisodeHarvest(vec, A * B, env // per)
    # rows of opponent b: its block under every agent
    rows_of = [torch.cat([env[(a * B + b) * per:(a * B + b + 1) * per] for a in range(A)]) for b in range(B)]
    acts = torch.zeros((E, vec.N_AGENTS), dtype=torch.int8, device=dev)
    n_steps = min(int(vec.cfg.game_steps), int(max_steps) + 1)
    recorder = None
    if record is not None:
        k = int(record)
        if k < 1 or k > per:
            raise ValueError(f"record = {record}: a pairing's block has {per} envs")
        recorder = StateRecorder(vec, [g * per + j for g in range(A * B) for j in range(k)], n_steps + 1)
    vec.reset()
    if recorder:
        recorder.record()
    with torch.no_grad():
        for _ in range(n_steps):
            obs, meta = vec.observe()
            for a, net in enumerate(agents):
                sl = slice(a * B * per, (a + 1) * B * per)
                acts[sl][:, col.trained_idx] = col._policy(net, obs[sl], meta[sl], col.trained_idx)[0].to(torch.int8).transpose(0, 1)
            for b, net in enumerate(opponents):
                rows = rows_of[b]
                if isinstance(net, ScriptedPolicy):
                    continue
                act = col._policy(net, obs.index_select(0, rows), meta.index_select(0, rows), col.others_idx)[0]
                acts[rows[:, None], col.others_idx[None, :]] = act.to(torch.int8).transpose(0, 1)
            mapped = col.rev_lut[acts.long()]  # team-1 agents act in their flipped view (utils.py:535-551)
            joint = torch.where(col.is_team1[None, :], mapped, acts).contiguous()
            for b, net in enumerate(opponents):
                if isinstance(net, ScriptedPolicy):  # env actions: written behind the mapping
                    rows = rows_of[b][:, None]
                    joint[rows, col.others_idx[None, :]] = net.act(vec, col.others_mask)[rows, col.others_idx[None, :]]
            vec.step(joint)
            if recorder:
                recorder.record()
    harvest.update(all_envs=True)
    table = harvest.table()
    episodes = table[:, 0].reshape(A, B)
    counts = table[:, 1:4].reshape(A, B, 3)
    out = dict(episodes=episodes, result_counts=counts, win_rate=counts[:, :, 0] / np.maximum(episodes, 1), table=table, steps=n_steps)
    if visitation:
        out["visitation"] = harvest.visitation_table().reshape(A, B, vec.N_AGENTS, vec.GRID_SIZE, vec.GRID_SIZE)
    if recorder:
        fr = recorder.frames()
        out["trajectories"] = [[[frames_to_trajectory(vec, fr, (a * B + b) * k + j) for j in range(k)] for b in range(B)] for a in range(A)]
    return out


def duel_trajectory(vec, agent, opponent, env_index=0, max_steps=256):
    """The three.js viewer record of ``utils.duel_json`` (reference utils.py:728-815) for ONE env of a batched duel:
    static map, per-step position deltas + ``has_flag``, destructible tiles and scores — the same dict, key for key
    (the reference also dumps it to a file; pass the result to ``json.dump``)."""
    import numpy as np
    import torch

    col = BatchedRolloutCollector(vec, 1, 0)
    use_codes = col.use_codes(agent, opponent)
    n, g = vec.N_AGENTS, vec.GRID_SIZE
    scen = vec.derived["kwargs"]["SCENARIO"]
    vec.reset()

    def snapshot():
        v = vec.get_state(env_index)
        grid = np.frombuffer(v.grid, dtype=np.uint8, count=g * g).reshape(g, g)
        pos = [(int(v.pos[i][0]), int(v.pos[i][1])) for i in range(n)]
        return grid, pos, [int(v.has_flag[i]) for i in range(n)], (int(v.team_captures[0]), int(v.team_captures[1]))

    def tiles_of(grid):
        return [{"x": int(x), "z": int(z), "type": 0} for z, x in zip(*np.where(grid == 2))] + \
               [{"x": int(x), "z": int(z), "type": 1} for z, x in zip(*np.where(grid == 3))]

    grid, pos, _, _ = snapshot()
    out = {
        "grid_size": g,
        "flag_pos": {f"{k}": {"x": v[1], "z": v[0]} for k, v in scen["FLAG_POSITIONS"].items()},
        "spawn_pos": {f"{k}": {"x": v[1], "z": v[0]} for k, v in scen["SPAWN_POSITIONS"].items()},
        "agent_config": [{"team": vec.AGENT_TEAMS[i], "type": vec.AGENT_TYPES[i], "start_x": scen["AGENT_STARTING_POSITIONS"][i][1],
                          "start_z": scen["AGENT_STARTING_POSITIONS"][i][0]} for i in range(n)],
        "block_tiles": [{"x": int(x), "z": int(z)} for z, x in zip(*np.where(grid == 1))],
        "destructible_tiles": tiles_of(grid),
    }
    movement, tiles, scores = [], [], []
    n_steps = min(int(vec.cfg.game_steps), int(max_steps) + 1)
    with torch.no_grad():
        for _ in range(n_steps):
            vec.step(col.joint_actions(agent, opponent, use_codes)[1])
            grid, new_pos, has_flag, caps = snapshot()
            movement.append([{"x": new_pos[i][1] - pos[i][1], "z": new_pos[i][0] - pos[i][0], "has_flag": has_flag[i]} for i in range(n)])
            tiles.append(tiles_of(grid))
            scores.append([{"t0": caps[0], "t1": caps[1]}])
            pos = new_pos
    out["movement"], out["tiles"], out["scores"] = movement, tiles, scores
    return out


def duel_trajectories(vec, agent, opponent, env_indices, max_steps=256):
    """``duel_trajectory`` for SEVERAL envs of one batched duel: the envs' states are recorded on the device, one
    ``frames.StateRecorder`` launch per step instead of one ``get_state`` round trip per env and step, and decoded on the host after
    the last step.  -> a list of dicts, entry j the record of env ``env_indices[j]`` (repeats allowed)."""
    import torch

    col = BatchedRolloutCollector(vec, 1, 0)
    use_codes = col.use_codes(agent, opponent)
    n_steps = min(int(vec.cfg.game_steps), int(max_steps) + 1)
    recorder = StateRecorder(vec, env_indices, n_steps + 1)
    vec.reset()
    recorder.record()
    with torch.no_grad():
        for _ in range(n_steps):
            vec.step(col.joint_actions(agent, opponent, use_codes)[1])
            recorder.record()
    fr = recorder.frames()
    return [frames_to_trajectory(vec, fr, j) for j in range(recorder.n)]
