"""The MPC loss's terms as data: pressure bounds, the constraint's weight, alpha (include/fcr.h fcr_loss_terms).

For horizon step j and the surrogate's scaled prediction x̂_j = (ẏ, p1, p2, z) the loss adds
``w · (relu(p1_lo − p1) + relu(p2_lo − p2) + relu(p1 − p1_hi) + relu(p2 − p2_hi))`` to the tracking error and
``alpha · Δu²``. The reference hard-wires the bounds to 32e6 Pa over ITS output scaler's ``max_abs_`` (Functions.py:1411),
lower bounds 0 and weight 1; :class:`LossTerms` carries them, and :meth:`LossTerms.from_scalers` derives them from a
scaler and bounds in Pa — the numbers :class:`~.closed_loop.FeasibilityRecovery` and ``ClosedLoopBank.run`` take.
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass

from ._native import P1_MAX, P2_MAX


def _pair(name, v):
    try:
        lo, hi = (float(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(f"LossTerms: {name} must be a (lo, hi) pair of numbers, got {v!r}") from None
    if math.isnan(lo) or math.isnan(hi):
        raise ValueError(f"LossTerms: {name} = ({lo}, {hi}) holds a NaN")
    if lo > hi:
        raise ValueError(f"LossTerms: {name} lower bound {lo} is above its upper bound {hi}")
    return lo, hi


@dataclass(frozen=True)
class LossTerms:
    """``p1`` / ``p2``: (lo, hi) bounds of the scaled pressures (``-inf`` / ``+inf`` switch a side off); ``weight``:
    the constraint's weight (>= 0); ``alpha``: the command cost's weight, None = the loss's own ``alpha``. The
    defaults are the reference's loss, bit for bit. NaN, ``lo > hi`` and a negative weight raise ``ValueError``."""

    p1: tuple = (0.0, P1_MAX)
    p2: tuple = (0.0, P2_MAX)
    weight: float = 1.0
    alpha: float | None = None

    def __post_init__(self):
        object.__setattr__(self, "p1", _pair("p1", self.p1))
        object.__setattr__(self, "p2", _pair("p2", self.p2))
        w = float(self.weight)
        if not (w >= 0.0 and math.isfinite(w)):
            raise ValueError(f"LossTerms: weight = {self.weight!r} must be finite and >= 0")
        object.__setattr__(self, "weight", w)
        if self.alpha is not None:
            a = float(self.alpha)
            if not math.isfinite(a):
                raise ValueError(f"LossTerms: alpha = {self.alpha!r} must be finite (or None: the loss's own)")
            object.__setattr__(self, "alpha", a)

    def replace(self, **changes) -> "LossTerms":
        return dataclasses.replace(self, **changes)

    def as_row(self, alpha: float) -> tuple:
        """``(alpha, p1_lo, p1_hi, p2_lo, p2_hi, weight)``: a row of the kernels' table; ``alpha`` fills in for None."""
        return (float(self.alpha if self.alpha is not None else alpha), self.p1[0], self.p1[1], self.p2[0], self.p2[1],
                self.weight)

    @classmethod
    def from_scalers(cls, output_scaler, p1_pa=(0.0, 32e6), p2_pa=(0.0, 32e6), weight=1.0, alpha=None) -> "LossTerms":
        """Bounds in Pa over the surrogate's output scaling: ``output_scaler`` is a fitted ``MaxAbsScaler`` (its
        ``max_abs_``) or the 4-vector itself, in the order (ẏ, p1, p2, z)."""
        m = getattr(output_scaler, "max_abs_", output_scaler)
        m = [float(v) for v in m]
        if len(m) != 4 or not all(v > 0.0 and math.isfinite(v) for v in m):
            raise ValueError(f"LossTerms.from_scalers: expected four positive max_abs_ values, got {m}")
        return cls(p1=(float(p1_pa[0]) / m[1], float(p1_pa[1]) / m[1]), p2=(float(p2_pa[0]) / m[2], float(p2_pa[1]) / m[2]),
                   weight=weight, alpha=alpha)


def resolve(terms, n_models=None):
    """``MPCLoss(terms=...)`` checked: None, one :class:`LossTerms`, or (banks) a sequence of them -> a tuple."""
    if terms is None or isinstance(terms, LossTerms):
        return terms
    seq = tuple(terms)
    if not seq or not all(isinstance(t, LossTerms) for t in seq):
        raise TypeError("MPCLoss: terms must be a LossTerms or a non-empty sequence of LossTerms (one per bank model)")
    if n_models is not None and len(seq) != n_models:
        raise ValueError(f"MPCLoss: {len(seq)} LossTerms for a bank of {n_models} models")
    return seq
