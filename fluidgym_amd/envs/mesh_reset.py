"""``reset_mesh_envs``, ``set_mesh_state_bank`` / ``mesh_state_bank`` and ``record_mesh_state_bank`` of the multi-block envs (cylinder,
airfoil): chosen envs of a batch start a new episode from a stored state, and no other env is touched -- what ``reset_envs`` gives
the single-block envs, under names of their own.  A chosen env becomes a state of the ``MeshStateBank``, on the 3-D
envs mirrored and rolled along the span, with the family's reset noise from a counter-based stream when randomising: one launch
(``MultiBlockDomain.RestoreEnvs``).  The stream of env ``e`` is numbered by ``mesh_reset_count[e]``, which counts the per-env resets
of that env since the last ``reset(seed=...)`` and travels in ``get_state()`` (under ``"extra"``, beside the last control).

What differs from ``reset``: no warm-up simulation steps are run (they would advance the other envs too) -- a bank recorded over a
shedding period (``record_mesh_state_bank``) stands in for them --, the noise is not projected onto divergence-free fields (the
first step's pressure correction does that), and the pressure is rolled with the velocity."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch


class MeshResetMixin:
    _mesh_state_bank = None
    _mesh_state_bank_explicit = False
    _mesh_state_bank_mode = None
    _mesh_reset_count: Optional[np.ndarray] = None
    _mesh_reset_sigma: float = 0.0      # amplitude of the family's _randomize_domain noise on velocity and pressure

    def _mesh_reset_warmup_env_steps(self) -> int:
        """The longest warm-up of the family's ``_randomize_domain`` in env steps: what a recorded bank spans by default."""
        raise NotImplementedError

    @property
    def mesh_reset_count(self) -> np.ndarray:
        """Per env: how many ``reset_mesh_envs`` calls have chosen it since the last ``reset(seed=...)``."""
        if self._mesh_reset_count is None:
            self._mesh_reset_count = np.zeros(self._num_envs, dtype=np.int64)
        return self._mesh_reset_count

    @property
    def mesh_state_bank(self):
        """The ``MeshStateBank`` ``reset_mesh_envs`` restores from (None until one is set, recorded or built)."""
        return self._mesh_state_bank

    def set_mesh_state_bank(self, states, env: Optional[int] = None) -> None:
        """The states ``reset_mesh_envs`` restores from: a ``MeshStateBank``, or a list of ``get_state()`` /
        ``MultiBlockDomain.Clone()`` dicts (env ``env`` of each, or every env of every dict as an entry of its own); None returns to
        the bank built on demand."""
        from ..simulation.mb_state_bank import MeshStateBank

        self._mesh_state_bank = states if isinstance(states, MeshStateBank) or states is None else MeshStateBank(states, env=env)
        self._mesh_state_bank_explicit = states is not None

    def _require_mesh_reset(self, entry: str) -> None:
        from ..simulation.multiblock import MultiBlockDomain

        if not self._reset_called or self._domain is None:
            raise RuntimeError(f"Environment must be reset before {entry}(). Call 'reset()' first.")
        if not isinstance(self._domain, MultiBlockDomain):
            raise NotImplementedError(f"{entry} needs a multi-block domain (cylinder, airfoil envs); single-block envs have reset_envs")
        if self.heterogeneous:
            raise NotImplementedError(f"{entry} is not implemented for a batch with one parameter value per env: a stored state "
                                      "belongs to one Re")

    def _build_mesh_state_bank(self):
        """The bank of the first ``reset_mesh_envs`` without an explicit one: every initial domain of the current mode that is on
        disk (read once, the way ``load_initial_domain`` reads one), else env 0 of the state ``reset()`` starts from."""
        from ..simulation.domain_io import load_multiblock_domain
        from ..simulation.mb_state_bank import MeshStateBank
        from .fluid_env import N_INITIAL_DOMAINS

        if self._load_domain_on_reset and self._initial_domain_ids_on_disk():
            snaps = []
            for idx in range(N_INITIAL_DOMAINS):
                if not self._check_initial_domains_exists(mode=self._mode, idx=idx):
                    continue
                path = self._get_domain_dir(idx) / self._mode.value
                loaded = load_multiblock_domain(str(path), device=self._cuda_device, batch=1, dtype=self._dtype)
                try:
                    if loaded.n_cells != self._domain.n_cells or [b.size for b in loaded.blocks] != [b.size for b in self._domain.blocks]:
                        raise ValueError(f"initial domain {path} does not match this environment's mesh")
                    snaps.append(loaded.Clone())
                finally:
                    loaded.close()
            if snaps:
                return MeshStateBank(snaps, env=0)
        start = getattr(self, "_loaded_initial", None)
        if start is None:
            start = getattr(self, "_developed", None)
        if start is None:
            raise RuntimeError("reset_mesh_envs: no state bank, no initial domain on disk and no developed state; "
                               "call set_mesh_state_bank() or record_mesh_state_bank() first")
        return MeshStateBank([start], env=0)

    def record_mesh_state_bank(self, n_states: int, every: Optional[int] = None):
        """Record a bank of ``n_states`` phases of the uncontrolled flow and install it: from the current state, with the zero action
        on the boundary, env 0 is stored after every ``every``-th sim step, ``n_states`` times; then the saved state and the counters
        are put back.  Default ``every``: the span of the family's ``_randomize_domain`` warm-up spread evenly over ``n_states``,
        never below 1.  It is not an episode: recorders and tracer clouds are not sampled."""
        from ..simulation.mb_state_bank import FIELDS, MeshStateBank

        self._require_mesh_reset("record_mesh_state_bank")
        n_states = int(n_states)
        if n_states < 1:
            raise ValueError(f"record_mesh_state_bank: n_states must be at least 1, got {n_states}")
        if every is None:
            every = max(1, (self._mesh_reset_warmup_env_steps() * self._n_sim_steps) // n_states)
        every = int(every)
        if every < 1:
            raise ValueError(f"record_mesh_state_bank: every must be at least 1, got {every}")
        dom, sim = self._domain, self._sim
        saved = self.get_state()
        episode_steps = self.episode_steps.copy()
        last_control, mirror = self._last_control, getattr(self, "_last_control_mirror", None)
        clock = (sim.total_time, sim.total_step, sim.last_substeps, sim.last_iterations)
        snaps = []
        try:
            self._apply_action(self._zero_action.reshape(self._num_envs, *self._zero_action.shape[self._batched:]))
            for _ in range(n_states):
                for _ in range(every):
                    sim.single_step()
                snaps.append({k: getattr(dom, k)[0:1].clone() for k in FIELDS})
        finally:
            self.set_state(saved)
            self.episode_steps[:] = episode_steps
            self._last_control, self._last_control_mirror = last_control, mirror
            sim.total_time, sim.total_step, sim.last_substeps, sim.last_iterations = clock
        bank = MeshStateBank(snaps)
        self.set_mesh_state_bank(bank)
        return bank

    def reset_mesh_envs(self, envs, randomize: Optional[bool] = None):
        """Start a new episode in the envs ``envs`` (a sequence of indices or a bool mask ``[num_envs]``) and in no other; returns
        the observation at batch shape.  Each chosen env is restored from the mesh state bank (``set_mesh_state_bank``,
        ``record_mesh_state_bank``; without one the initial domains on disk for the current mode, else env 0 of the state
        ``reset()`` starts from) by ONE kernel launch.  With ``randomize`` (default: the env's ``randomize_initial_state``) the
        draws are made for each chosen env in ascending index order from the env's NumPy generator -- the source state when the
        bank holds more than one, then on the 3-D envs a mirror and a roll along the span -- and the family's reset noise is added
        from the counter-based stream of (seed, env, ``mesh_reset_count[env]``).  The zero action is then applied to the chosen
        envs' boundary values, their ``_last_control`` and ``episode_steps`` return to zero, and their tracers to their seeds."""
        from ..simulation.state_bank import draw_reset_plan, normalize_envs

        self._require_mesh_reset("reset_mesh_envs")
        chosen = normalize_envs(envs, self._num_envs)
        randomize = self._randomize_initial_state if randomize is None else bool(randomize)
        if self._mesh_state_bank is None or (not self._mesh_state_bank_explicit and self._mesh_state_bank_mode != self._mode):
            self._mesh_state_bank, self._mesh_state_bank_mode = self._build_mesh_state_bank(), self._mode
        bank, dom = self._mesh_state_bank, self._domain
        nz = dom.span_nz()
        plan = draw_reset_plan(self._np_rng, chosen, bank.size, ("flip_z", "shift_z") if nz else (), 1, nz or 1, randomize)
        count = self.mesh_reset_count
        noise = None
        if randomize:
            sigma = float(self._mesh_reset_sigma)
            noise = (self._seed, sigma, sigma, [int(count[e]) for e in plan["env"]])
        self._last_reset_noise = noise
        dom.RestoreEnvs(bank, plan["env"], plan["src"], plan["flip_z"], plan["shift_z"], noise=noise)
        count[chosen] += 1
        self._last_reset_plan = plan
        idx = torch.as_tensor(chosen, dtype=torch.int64, device=self._cuda_device)
        # the zero action on the chosen envs' boundary values only: the boundary rows of the other envs are put back
        others = torch.as_tensor(sorted(set(range(self._num_envs)) - set(chosen)), dtype=torch.int64, device=self._cuda_device)
        if others.numel():
            saved = dom.boundary_velocity.index_select(0, others)
        self._apply_action(self._zero_action.reshape(self._num_envs, *self._zero_action.shape[self._batched:]))
        if others.numel():
            dom.boundary_velocity.index_copy_(0, others, saved)
        control = self._last_control.clone()
        control[idx] = 0
        self._last_control, self._last_control_mirror = control, None
        self._reseed_hooks(chosen)
        self.episode_steps[chosen] = 0
        obs = self._get_local_obs() if self._use_marl else self._get_global_obs()
        return self._unbatch(obs)

    # ---- the counter: zeroed by a seeded reset; the env carries it in its extra state (MeshBodyEnvBase._get_extra_state)
    def reset(self, seed: Optional[int] = None, randomize: Optional[bool] = None, per_env: bool = False):
        if seed is not None:
            self.mesh_reset_count[:] = 0
        return super().reset(seed=seed, randomize=randomize, per_env=per_env)
