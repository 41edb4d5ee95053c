"""Exploring starts for a batch: ``ScatteredStarts`` holds the arguments of ``VecGridworldCtf.reset_scattered`` and the per-env episode
counters that make every reset draw afresh (include/ctf_env.h, ctf_reset_scattered).

    starts = ScatteredStarts(radius=2, own_side=True, seed=7)
    starts.reset(vec)               # every env: agents drawn round their start cells
    ...
    starts.reset(vec, mask=done)    # behind the harvests: the finished envs start their next episode somewhere else

``BatchedRolloutCollector.collect(..., starts=starts)`` uses it in place of ``vec.reset()``.  The reference has no such reset, and
``vec.step(auto_reset=True)`` still goes to the config's start cells: a loop that wants scattered starts steps without auto-reset."""


class ScatteredStarts:
    def __init__(self, radius, own_side=False, agent_mask=None, team=None, seed=0):
        if int(radius) < 0:
            raise ValueError("radius must be >= 0")
        if agent_mask is not None and team is not None:
            raise ValueError("give agent_mask or team, not both")
        self.radius, self.own_side, self.agent_mask, self.team, self.seed = int(radius), bool(own_side), agent_mask, team, int(seed)
        self._episodes = {}  # id(vec) -> (vec, uint32 [E] on its device): allocated at the vec's first reset, then advanced by the kernel

    def episodes(self, vec):
        """the episode counters of ``vec``'s envs (uint32 [E], zeros at first): how often each env has been reset through this object"""
        entry = self._episodes.get(id(vec))
        if entry is None or entry[0] is not vec:
            import torch

            entry = (vec, torch.zeros((vec.n_envs,), dtype=torch.uint32, device=vec.device))
            self._episodes[id(vec)] = entry
        return entry[1]

    def reset(self, vec, mask=None, env_offset=0):
        """one launch: ``vec.reset_scattered`` for the envs of ``mask`` (uint8 [E], None = all) with this object's arguments and counters"""
        vec.reset_scattered(mask=mask, radius=self.radius, agent_mask=self.agent_mask, team=self.team, own_side=self.own_side, seed=self.seed, round=0,
                            episodes=self.episodes(vec), env_offset=env_offset)
