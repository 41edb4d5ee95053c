"""Potential-based reward shaping from the scripted planners' cost-to-go (include/ctf_env.h, ctf_scripted_costs).

The reference's reward is sparse (a capture pays 1, everything else 0 by default).  A shaping term of the form
``F = gamma * Phi(s') - Phi(s)`` leaves the optimal policy alone (Ng, Harada and Russell, 1999), whatever ``Phi`` is; a useful
``Phi`` says how far an agent is from what pays.  Here ``Phi = -scale * min(cost, cap)`` with ``cost`` the path cost a scripted bot
of the agent's role and class would have to pay from the state — it knows walls, destructible tiles, jumps and other agents, which
a Chebyshev distance to the flag does not — computed on the device by one launch per step.
"""


class PotentialShaping:
    """``bot``: a ``ScriptedPolicy`` / ``ScriptedTeam`` (anything with ``costs(vec, agent_mask, out=None) -> int16 [E, N]``): its roles
    and abilities define the potential.  ``agent_mask``: the agents that are shaped (bit i = agent i); every other agent's column of
    ``step``'s result is 0.  ``gamma``: the learner's discount.  ``cap``: costs are clipped to it and ``CTF_COST_NONE`` (no way to
    the goal) counts as ``cap``; None: ``4 * G`` — a default (a few grid widths, so that detours still register and an unreachable
    goal is finite), not a tuned value.

    ``begin(vec)`` behind a reset of the whole batch, then ``step(vec, done)`` behind every ``vec.step``:

        Phi'     = where(done, 0, Phi(s'))           a terminal state has potential 0
        F        = gamma * Phi' - Phi_prev
        Phi_prev = where(done & auto_reset, Phi_start, Phi')

    Without auto-reset an env that runs on past its end then gets F = 0.  With auto-reset the next episode starts from ``Phi_start``,
    the potential ``begin`` saw: ``step(auto_reset=True)`` ASSUMES CONFIG STARTS — the in-kernel reset, like ``ctf_reset``, draws
    nothing and restores the config's start cells, so an auto-reset episode starts in the state ``begin`` saw when that was a plain
    ``reset``.  ``Phi_start`` is kept per env, so ``begin`` behind ``reset_scattered`` (``collect(starts=...)``, which steps without
    auto-reset) is as exact: every env's first F is measured from its own start.
    With gamma = 1 the F of an episode sum to ``scale * min(cost(s0), cap)`` exactly."""

    def __init__(self, bot, agent_mask, gamma=0.99, scale=1.0, cap=None):
        if int(agent_mask) < 0:
            raise ValueError("agent_mask must not be negative")
        if cap is not None and not 0 <= int(cap) < 32768:
            raise ValueError("cap must be in 0..32767 (costs are int16)")
        self.bot, self.agent_mask = bot, int(agent_mask)
        self.gamma, self.scale = float(gamma), float(scale)
        self.cap = None if cap is None else int(cap)
        self.phi_start = self.phi_prev = None
        self._cost = self._cols = None

    def potential(self, vec):
        """Phi of the batch's present state -> float32 [E, N] (a new tensor), 0 for the agents outside the mask"""
        import torch

        self._cost = self.bot.costs(vec, self.agent_mask, out=self._cost)
        cost = self._cost
        if self._cols is None:
            if self.agent_mask >> cost.shape[1]:
                raise ValueError(f"agent_mask 0x{self.agent_mask:x} names an agent outside 0..{cost.shape[1] - 1}")
            self._cols = torch.tensor([(self.agent_mask >> i) & 1 == 1 for i in range(cost.shape[1])], device=cost.device)
            if self.cap is None:
                self.cap = 4 * int(vec.GRID_SIZE)
        capped = torch.where(cost < 0, torch.full_like(cost, self.cap), cost.clamp(max=self.cap)).to(torch.float32)
        return torch.where(self._cols[None, :], -self.scale * capped, torch.zeros_like(capped))

    def begin(self, vec):
        """``vec`` must be a freshly reset batch (every env in its start state): keeps Phi_start and sets Phi_prev to it"""
        self.phi_start = self.potential(vec)
        self.phi_prev = self.phi_start.clone()
        return self

    def step(self, vec, done, auto_reset=False):
        """behind ``vec.step(..., auto_reset=auto_reset)`` with that step's ``done`` [E] -> F float32 [E, N] (a new tensor)"""
        import torch

        if self.phi_prev is None:
            raise RuntimeError("PotentialShaping.step before begin")
        over = done.to(torch.bool)[:, None]
        phi = torch.where(over, torch.zeros_like(self.phi_prev), self.potential(vec))
        f = self.gamma * phi - self.phi_prev
        self.phi_prev = torch.where(over, self.phi_start, phi) if auto_reset else phi
        return f
