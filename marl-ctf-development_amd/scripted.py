"""Scripted opponents: a baseline that sits where a network sits — the ``opponent`` of ``batched_duel``, any entry of
``batched_tournament``'s ``opponents``, the ``opponent`` of ``BatchedRolloutCollector.collect`` — and is computed on the device
from the env state by one launch (include/ctf_env.h, ctf_scripted_actions), so that a win rate has a fixed anchor and a league
something to start against.

A ``ScriptedPolicy`` is not a network: it has no ``get_action_and_value``, reads no observation and launches no policy kernel.  Its
actions are ENV actions (the state is read, not a team-1 agent's flipped view): the collectors hand them to ``vec.step`` as they
are, NOT through ``REVERSED_ACTION_MAP``.
"""
try:
    from . import _abi
except ImportError:  # pragma: no cover
    import _abi


class ScriptedPolicy:
    """kind "runner": every agent takes a shortest open path to a cell next to the flag it wants — the other team's, or its own once
    it carries one — (breadth-first over open cells; agents, flags and blocks are walls; ties go to the lowest action).
    ``epsilon``: probability of a uniform move on 0..4 instead, from a Philox stream keyed by ``seed`` and indexed by (env, call,
    agent): the same object replays the same games after ``restart()``.  ``abilities``: False keeps the walking bot (today's calls and
    bytes); True, a bit mask or a sequence of agent indices routes through ``VecGridworldCtf.scripted_abilities``: the named agents
    (True: all) plan with their type's movement ability — miners dig, vaulters jump."""

    def __init__(self, kind="runner", epsilon=0.0, seed=0, abilities=False):
        if kind not in _abi.SCRIPT_KINDS:
            raise ValueError(f"kind must be one of {sorted(_abi.SCRIPT_KINDS)}")
        if not 0.0 <= float(epsilon) <= 1.0:
            raise ValueError("epsilon must be in [0, 1]")
        self.kind, self.epsilon, self.seed = kind, float(epsilon), int(seed)
        self.abilities = abilities
        self.calls = 0  # the exploration stream's step index: one per decision

    def restart(self):
        self.calls = 0

    def act(self, vec, agent_mask, out=None, env_offset=0):
        """One decision of the agents of ``agent_mask`` in every env of ``vec``, written into ``out`` (int8 [E, N]) in place."""
        if self.abilities is False:
            out = vec.scripted_actions(agent_mask=agent_mask, out=out, epsilon=self.epsilon, seed=self.seed, step=self.calls, kind=self.kind,
                                       env_offset=env_offset)
        else:
            out = vec.scripted_abilities([self.kind] * vec.N_AGENTS, self._ability_arg(), agent_mask=agent_mask, out=out, epsilon=self.epsilon,
                                         seed=self.seed, step=self.calls, env_offset=env_offset)
        self.calls += 1
        return out

    def costs(self, vec, agent_mask, out=None):
        """The cost-to-go of the agents of ``agent_mask`` under this bot's own rules (``VecGridworldCtf.scripted_costs`` with its roles
        and abilities) -> int16 [E, N], only the asked entries of ``out`` written.  A function of the state: no exploration, and
        ``calls`` does not advance."""
        return vec.scripted_costs(self._role_arg(vec), self.abilities, agent_mask=agent_mask, out=out)

    def _role_arg(self, vec):
        return None  # all runners

    def _ability_arg(self):
        return None if self.abilities is True else self.abilities


class ScriptedTeam(ScriptedPolicy):
    """A bot with a ROLE per agent (``VecGridworldCtf.scripted_roles``): ``roles`` is a sequence of N names of "runner", "chaser" and
    "guard", a dict agent -> name (the rest run), or a callable ``cfg -> roles`` resolved against ``vec.cfg`` at the first ``act``
    (``guardians_guard`` below).  It sits wherever a ``ScriptedPolicy`` sits; the agents it decides for are the caller's
    ``agent_mask``, so one object serves either team.  ``abilities``: as for ``ScriptedPolicy``."""

    def __init__(self, roles, epsilon=0.0, seed=0, abilities=False):
        super().__init__("runner", epsilon, seed, abilities)
        self.roles = roles
        self._resolved = None

    def _role_arg(self, vec):
        if self._resolved is None:
            self._resolved = self.roles(vec.cfg) if callable(self.roles) else self.roles
        return self._resolved

    def act(self, vec, agent_mask, out=None, env_offset=0):
        self._role_arg(vec)
        if self.abilities is False:
            out = vec.scripted_roles(self._resolved, agent_mask=agent_mask, out=out, epsilon=self.epsilon, seed=self.seed, step=self.calls,
                                     env_offset=env_offset)
        else:
            out = vec.scripted_abilities(self._resolved, self._ability_arg(), agent_mask=agent_mask, out=out, epsilon=self.epsilon, seed=self.seed,
                                         step=self.calls, env_offset=env_offset)
        self.calls += 1
        return out


class ScriptedWanderer(ScriptedPolicy):
    """A random opponent that never bumps into a wall (``VecGridworldCtf.random_effective_actions``): every decision is a uniform
    draw among the actions that DO something in the state as it stands — a move into an open cell, a jump the hp pays for, a hit on a
    destructible tile, a block the inventory and the spawn windows allow — from a Philox stream keyed by ``seed`` and indexed by
    (env, call, agent); an agent with no such action stays.  It sits wherever a ``ScriptedPolicy`` sits and replays the same games
    after ``restart()``.  It has no goal, so it has no cost-to-go."""

    def __init__(self, seed=0):
        super().__init__("runner", 0.0, seed, False)

    def act(self, vec, agent_mask, out=None, env_offset=0):
        if out is None:
            if getattr(vec, "_scripted_out", None) is None:  # the buffer ``scripted_actions`` hands out (zero where never written)
                import torch

                vec._scripted_out = torch.zeros((vec.n_envs, vec.N_AGENTS), dtype=torch.int8, device=vec.device)
            out = vec._scripted_out
        out = vec.random_effective_actions(out, self.seed, self.calls, agent_mask=agent_mask, env_offset=env_offset)
        self.calls += 1
        return out

    def costs(self, vec, agent_mask, out=None):
        raise NotImplementedError("a wanderer has no goal: there is no cost-to-go")


def guardians_guard(cfg):
    """roles for ``ScriptedTeam``: the agents of type 1 (guardians: they hit harder near their own flag) guard, the rest run"""
    return ["guard" if int(cfg.agent_type[i]) == 1 else "runner" for i in range(cfg.n_agents)]
