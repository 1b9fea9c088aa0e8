"""The description of a per-env unsteady inflow -- gusts -- as ``MultiBlockDomain.ApplyInflowDisturbance`` and the cylinder and airfoil
envs take it (``fg_mb_inflow_disturbance``, csrc/fg_mb_inflow.hip).  Env b's inflow is its steady base profile times

    u = base_u (1 + S_b(t)),  v = base_v + base_u G_b(t, y)
    S_b = sum_k a_k sin 2 pi (f_k t + phi_k),   G_b = sum_k g_k sin 2 pi (h_k t + psi_k - kappa y)

with up to 8 modes each.  Two forms: tables of modes (one row for every env, or one per env), and the random form, whose modes the
kernel draws per env and per episode from a counter-based stream of (seed, env_offset + b, episode).  The description holds no
running state: the time of env b is its own sim-step count, the episode its own reset count, and both are the env's."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

MAX_MODES = 8
MAX_STREAMWISE_SUM = 0.9      # sum_k |a_k| above this could reverse the inflow
_TABLE_KEYS = ("a", "f", "phi", "g", "h", "psi")


def _table(v, name: str) -> np.ndarray:
    t = np.zeros((1, 0)) if v is None else np.atleast_2d(np.asarray(v, dtype=np.float64))
    if t.ndim != 2:
        raise ValueError(f"InflowDisturbance: {name} must be [K] or [B, K], got shape {np.shape(v)}")
    if t.shape[1] > MAX_MODES:
        raise ValueError(f"InflowDisturbance: {name} has K = {t.shape[1]} modes, at most {MAX_MODES}")
    if not np.isfinite(t).all():
        raise ValueError(f"InflowDisturbance: {name} is not finite")
    return t


class InflowDisturbance:
    """``InflowDisturbance(a, f, phi, g, h, psi, kappa=0.0)``: mode tables, each ``[K]`` (every env the same) or ``[B, K]``; the
    streamwise triple and the transverse triple may have different ``K`` (either may be left out).  ``InflowDisturbance.random(...)``:
    the drawn form.  ``ValueError`` when ``sum_k |a_k|`` exceeds 0.9 for an env (the inflow must never reverse), for more than 8 modes,
    and for a frequency that is negative or not finite."""

    def __init__(self, a=None, f=None, phi=None, g=None, h=None, psi=None, kappa: float = 0.0):
        self.form = "tables"
        self.tables = {k: _table(v, k) for k, v in zip(_TABLE_KEYS, (a, f, phi, g, h, psi))}
        for trio in (("a", "f", "phi"), ("g", "h", "psi")):
            shapes = {self.tables[k].shape[1] for k in trio}
            if len(shapes) != 1:
                raise ValueError(f"InflowDisturbance: {', '.join(trio)} must have the same number of modes")
        rows = {t.shape[0] for t in self.tables.values()} - {1}
        if len(rows) > 1:
            raise ValueError(f"InflowDisturbance: tables given per env disagree on the batch: {sorted(rows)}")
        self.batch: Optional[int] = rows.pop() if rows else None
        self.n_streamwise, self.n_transverse = self.tables["a"].shape[1], self.tables["g"].shape[1]
        if (self.tables["f"] < 0).any() or (self.tables["h"] < 0).any():
            raise ValueError("InflowDisturbance: frequencies must be non-negative")
        worst = float(np.abs(self.tables["a"]).sum(axis=1).max()) if self.n_streamwise else 0.0
        if worst > MAX_STREAMWISE_SUM:
            raise ValueError(f"InflowDisturbance: sum |a_k| = {worst:.4g} exceeds {MAX_STREAMWISE_SUM}: the inflow could reverse")
        self.kappa = self._finite(kappa, "kappa")
        self.seed, self.band, self.streamwise_rms, self.transverse_rms, self.env_offset = 0, (0.0, 0.0), 0.0, 0.0, 0
        self._device_modes: dict = {}

    @staticmethod
    def _finite(v, name: str) -> float:
        v = float(v)
        if not np.isfinite(v):
            raise ValueError(f"InflowDisturbance: {name} is not finite")
        return v

    @classmethod
    def random(cls, seed: int, n_streamwise: int = 4, n_transverse: int = 0, band: Sequence[float] = (0.05, 0.5),
               streamwise_rms: float = 0.05, transverse_rms: float = 0.0, kappa: float = 0.0, env_offset: int = 0) -> "InflowDisturbance":
        """Modes drawn per env and per episode: mode k of ``n_streamwise`` has its frequency in the k-th of ``n_streamwise`` equal
        parts of ``band`` and a uniform phase, every amplitude is ``streamwise_rms sqrt(2 / n_streamwise)`` (so the signal has that
        rms); the transverse modes likewise.  A pure function of (seed, ``env_offset`` + env, episode): a batch of 64 at offset 0
        and four of 16 at offsets 0, 16, 32, 48 see the same gusts."""
        self = cls.__new__(cls)
        self.form = "random"
        self.tables, self.batch = None, None
        self.n_streamwise, self.n_transverse = int(n_streamwise), int(n_transverse)
        for name, k in (("n_streamwise", self.n_streamwise), ("n_transverse", self.n_transverse)):
            if not 0 <= k <= MAX_MODES:
                raise ValueError(f"InflowDisturbance.random: {name} = {k} is outside 0..{MAX_MODES}")
        lo, hi = (cls._finite(v, "band") for v in band)
        if lo < 0 or hi < lo:
            raise ValueError(f"InflowDisturbance.random: band = ({lo}, {hi}) must satisfy 0 <= low <= high (frequencies are non-negative)")
        self.band = (lo, hi)
        self.streamwise_rms, self.transverse_rms = cls._finite(streamwise_rms, "streamwise_rms"), cls._finite(transverse_rms, "transverse_rms")
        if self.streamwise_rms < 0 or self.transverse_rms < 0:
            raise ValueError("InflowDisturbance.random: an rms amplitude is negative")
        worst = self.streamwise_rms * np.sqrt(2.0 * self.n_streamwise)       # K a_k
        if worst > MAX_STREAMWISE_SUM:
            raise ValueError(f"InflowDisturbance.random: sum |a_k| = {worst:.4g} exceeds {MAX_STREAMWISE_SUM}: the inflow could reverse")
        self.kappa = cls._finite(kappa, "kappa")
        self.seed, self.env_offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_offset)
        if not 0 <= self.env_offset < 2 ** 31:
            raise ValueError("InflowDisturbance.random: env_offset must be in [0, 2^31)")
        self._device_modes = {}
        return self

    def modes_table(self, batch: int) -> Optional[np.ndarray]:
        """The table form as the kernel reads it: ``[batch, 6, 8]`` doubles (rows a, f, phi, g, h, psi; unused columns zero); None in
        the random form."""
        if self.form == "random":
            return None
        if self.batch is not None and self.batch != int(batch):
            raise ValueError(f"InflowDisturbance: tables for a batch of {self.batch} on a batch of {batch}")
        out = np.zeros((int(batch), 6, MAX_MODES), dtype=np.float64)
        for i, k in enumerate(_TABLE_KEYS):
            t = self.tables[k]
            out[:, i, :t.shape[1]] = t
        return out

    def state_dict(self) -> dict:
        """Everything that defines the disturbance (plain Python and NumPy); there is no running state."""
        d = {"form": self.form, "kappa": self.kappa}
        if self.form == "tables":
            d["tables"] = {k: v.copy() for k, v in self.tables.items()}
        else:
            d.update(seed=self.seed, n_streamwise=self.n_streamwise, n_transverse=self.n_transverse, band=tuple(self.band),
                     streamwise_rms=self.streamwise_rms, transverse_rms=self.transverse_rms, env_offset=self.env_offset)
        return d

    def load_state_dict(self, d: dict) -> "InflowDisturbance":
        other = self.from_state_dict(d)
        self.__dict__.clear()
        self.__dict__.update(other.__dict__)
        return self

    @classmethod
    def from_state_dict(cls, d: dict) -> "InflowDisturbance":
        if d["form"] == "tables":
            return cls(**{k: v for k, v in d["tables"].items()}, kappa=d["kappa"])
        return cls.random(d["seed"], d["n_streamwise"], d["n_transverse"], d["band"], d["streamwise_rms"], d["transverse_rms"],
                          d["kappa"], d["env_offset"])
