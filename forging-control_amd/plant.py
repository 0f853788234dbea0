"""Batched forging-press plant on the GPU.

The reference integrates the press one trajectory at a time: CasADi's ``F = Ruge_Kuta(TS, f)``
(Functions.py:1743-1781, M = 4 RK4 sub-steps) over ``FeasibilityRecovery.forging_model``
(Functions.py:1615-1740), or do-mpc's simulator over ``template_model`` (template_model.py:19-149, whose
pressures are floored by ``smooth_relu``). :class:`ForgingRK4` is ``F`` for a whole batch of
trajectories: one fp64 HIP kernel (``fcr_plant_rk4``, forging-control_amd/csrc/fcr_plant.h) steps every
trajectory through S commands with its state kept in registers.
"""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np
import torch

from . import _native

STATE_NAMES = ("y", "y_dot", "p1", "p2", "z")     # template_model.py:66-70
TS_REFERENCE = 0.001                              # template_mpc.py:23 (controller t_step)
SUBSTEPS_REFERENCE = 4                            # Functions.py:1760


@dataclasses.dataclass(frozen=True)
class PressParams:
    """The 28 physical constants of ``forging_model`` / ``template_model`` under the reference's names
    (Functions.py:1636-1695); the defaults are the reference's values, the ones every call without parameters is
    compiled with. One set is one row of a parameter table: 28 fp64 values in the order of :attr:`NAMES`
    (``fcr_press``, include/fcr.h). The friction knee (0.5 m/s) and the smooth model's epsilon belong to the model's form
    and are not parameters."""
    M_MASS: float = 90000.0
    B_DAMP: float = 25000.0
    FT: float = 200000.0
    D1: float = 0.6
    D2: float = 0.5
    G: float = 9.81
    KB: float = 22e9
    V1_0: float = 0.3
    V2_0: float = 0.1
    KL_1: float = 8e-13
    KL_2: float = 14e-14
    CD: float = 0.63
    RHO: float = 858.0
    D: float = 0.006
    PS: float = 32e6
    PT: float = 101325.0
    MU: float = 0.3
    K: float = 1.115
    W0: float = 0.2
    H0: float = 0.5
    B0: float = 0.1
    T_DEF: float = 900.0
    T1: float = 0.005
    M0: float = 1200e6
    M1: float = -0.0025
    M2: float = -0.0587
    M3: float = 0.1165
    M4: float = -0.0065

    NAMES = ("M_MASS", "B_DAMP", "FT", "D1", "D2", "G", "KB", "V1_0", "V2_0", "KL_1", "KL_2", "CD", "RHO", "D", "PS", "PT",
             "MU", "K", "W0", "H0", "B0", "T_DEF", "T1", "M0", "M1", "M2", "M3", "M4")
    # the equations divide by these or take their root: they must be positive
    POSITIVE = ("M_MASS", "D1", "D2", "V1_0", "V2_0", "RHO", "W0", "H0", "B0", "T1")

    def replace(self, **kw) -> "PressParams":
        """A copy with the named fields changed."""
        return dataclasses.replace(self, **kw)

    def as_row(self) -> np.ndarray:
        """``(28,)`` fp64, the fields in the order of :attr:`NAMES`."""
        return np.array([getattr(self, n) for n in self.NAMES], dtype=np.float64)

    def struct(self) -> _native.FcrPress:
        return _native.FcrPress(*self.as_row())

    def table(self, n: int, device=None) -> torch.Tensor:
        """``(n, 28)`` fp64: this set for each of ``n`` trajectories."""
        return torch.tensor(np.tile(self.as_row(), (int(n), 1)), dtype=torch.float64, device=device)

    def sample(self, n: int, rel: dict, dist: str = "uniform", rng: np.random.RandomState | None = None,
               device=None) -> torch.Tensor:
        """``(n, 28)`` fp64: ``n`` presses around this one. ``rel`` maps a field name to a relative half-width
        (``dist="uniform"``: the field is this set's value times ``1 + U(-rel, rel)``) or a relative standard
        deviation (``"normal"``: times ``1 + rel * N(0, 1)``); fields ``rel`` does not name keep this set's value.

        Draw order (fixed): the named fields in the order of :attr:`NAMES` — not of ``rel`` — each as ONE call of
        ``rng.uniform(-1, 1, n)`` or ``rng.standard_normal(n)``. ``rng`` defaults to ``RandomState(0)``."""
        unknown = sorted(set(rel) - set(self.NAMES))
        if unknown:
            raise ValueError(f"PressParams.sample: unknown fields {unknown}; the fields are {self.NAMES}")
        if dist not in ("uniform", "normal"):
            raise ValueError(f"PressParams.sample: dist must be 'uniform' or 'normal', got {dist!r}")
        rng = np.random.RandomState(0) if rng is None else rng
        out = np.tile(self.as_row(), (int(n), 1))
        for i, name in enumerate(self.NAMES):
            if name in rel:
                z = rng.uniform(-1.0, 1.0, int(n)) if dist == "uniform" else rng.standard_normal(int(n))
                out[:, i] *= 1.0 + float(rel[name]) * z
        return torch.tensor(out, dtype=torch.float64, device=device)

    @classmethod
    def validate(cls, table: torch.Tensor) -> bool:
        """Whether every row of ``table (..., 28)`` is a press the equations can integrate: all fields finite and
        :attr:`POSITIVE`'s positive. One reduction (and one host read of its result); the kernels do not check."""
        if table.shape[-1] != len(cls.NAMES):
            raise ValueError(f"a parameter table has {len(cls.NAMES)} columns, got shape {tuple(table.shape)}")
        pos = torch.zeros(len(cls.NAMES), dtype=torch.bool, device=table.device)
        pos[[cls.NAMES.index(n) for n in cls.POSITIVE]] = True
        return bool((torch.isfinite(table) & ((table > 0) | ~pos)).all().item())


def as_press_table(params, device, what: str = "params") -> torch.Tensor:
    """``params`` (a :class:`PressParams`, or an array / tensor whose last dimension is 28) as a contiguous fp64 tensor
    on ``device``; an array's shape is kept."""
    if isinstance(params, PressParams):
        return torch.tensor(params.as_row(), dtype=torch.float64, device=device)
    t = torch.as_tensor(params)
    if t.dim() < 1 or t.shape[-1] != len(PressParams.NAMES):
        raise ValueError(f"{what}: the last dimension of a parameter table is {len(PressParams.NAMES)}, got {tuple(t.shape)}")
    if torch.is_tensor(params) and params.device != torch.device(device):
        raise RuntimeError(f"{what} must be on {device}, found it on {params.device}")
    return t.to(device=device, dtype=torch.float64).contiguous()


def forging_rk4(x0: torch.Tensor, u: torch.Tensor, ts: float = TS_REFERENCE,
                substeps: int = SUBSTEPS_REFERENCE, smooth: bool = False, params=None) -> torch.Tensor:
    """States of B trajectories under S held commands: x0 (B, 5), u (B, S) -> x (B, S+1, 5), fp64.

    ``x[:, 0] = x0`` and ``x[:, t+1] = F(x[:, t], u[:, t])`` with F the reference's RK4 integrator.
    ``smooth=True`` integrates template_model's dynamics (smooth_relu-floored pressures) instead of
    forging_model's. ``params``: the press — a :class:`PressParams` or a ``(28,)`` row for all trajectories, or a
    ``(B, 28)`` table, one row per trajectory (``fcr_plant_rk4_press``; a shared row is read through a zero stride, not
    expanded); ``None`` is the reference's press, the call as it always was. Runs on a ROCm device only; there is no CPU
    path.

    Differentiable: when ``x0`` or ``u`` requires grad (and grad mode is on) the result is attached to the graph; its
    values are the plain call's, bit for bit, and the backward is the hand-written adjoint of the RK4 step
    (``fcr_plant_rk4_vjp``, csrc/fcr_press_grad.h), which recomputes the sub-steps from the stored
    states. Conventions where the derivative is singular: the deformation force is differentiated only where ``y > 0``
    and ``y_dot > 0`` (at ``y_dot == 0`` its slope is infinite and is taken as 0, so a press at rest has finite
    gradients); the valve flow ``q = c z sign(a) sqrt(k|a|)`` has ``dq/da = dq/dz = 0`` at ``a == 0``, its branch chosen by
    ``z >= 0`` as in the forward; the friction's slope is ``FT/0.5`` where ``|y_dot| <= 0.5`` and 0 elsewhere; the smooth
    pressure floor's is ``0.5 (1 + p / sqrt(p^2 + eps))``. Gradients through this plant grow with S:
    back-propagation through hundreds of steps is the caller's risk.

    Gradients reach the press as well: when ``params`` is a ``(28,)`` or ``(B, 28)`` tensor that requires
    grad, the result is attached to it and the backward runs the adjoint's parameter-gradient kernels
    (``fcr_plant_rk4_vjp_press``); ``params.grad`` has the tensor's shape, dtype and device, for a ``(28,)`` row the sum
    over the trajectories, added in fp64 in a fixed order (``fcr_press_grad_sum``: two backward calls give the same
    bits). The same conventions hold for the parameters: the deformation fields (``MU, K, W0, H0, B0, T_DEF, M0..M4``)
    receive gradient only where ``y > 0`` and ``y_dot > 0``; ``CD, RHO, D, PS, PT`` receive 0 from a valve at a zero
    pressure difference, ``PS`` and ``PT`` by the branch ``z >= 0``; ``FT`` receives ``y_dot / 0.5`` inside the knee and
    1 outside. A :class:`PressParams` is a constant, and with ``params`` not requiring grad the call is what it was."""
    if u.dim() == 1:
        u = u.unsqueeze(1)
    if torch.is_grad_enabled() and (x0.requires_grad or u.requires_grad or _wants_grad(params)):
        return _ForgingRK4Grad.apply(x0, u, float(ts), int(substeps), bool(smooth), params)
    return _forging_rk4(x0, u, ts, substeps, smooth, params)[0]


def _wants_grad(params) -> bool:
    """Whether ``params`` is a tensor the graph follows (a PressParams, an array or None is a constant)."""
    return torch.is_tensor(params) and params.requires_grad


def press_grad_sum(g_press: torch.Tensor) -> torch.Tensor:
    """``(28,)`` fp64: the sum over the trajectories of ``g_press (B, 28)``, in a fixed order (``fcr_press_grad_sum``)."""
    B, dev = g_press.shape[0], g_press.device
    lib = _native.load()
    size = ctypes.c_size_t(0)
    _native.check(lib.fcr_press_grad_sum_workspace_size(B, ctypes.byref(size)), "fcr_press_grad_sum_workspace_size")
    ws = torch.empty(max(size.value, 8), dtype=torch.uint8, device=dev)
    g_row = torch.empty(28, dtype=torch.float64, device=dev)
    _native.check(lib.fcr_press_grad_sum(B, ctypes.c_void_p(g_press.data_ptr()), ctypes.c_void_p(g_row.data_ptr()),
                                         ctypes.c_void_p(ws.data_ptr()), ws.numel(), _native.stream(dev)),
                  "fcr_press_grad_sum")
    return g_row


def _forging_rk4(x0, u, ts, substeps, smooth, params):
    """The launch of :func:`forging_rk4`: ``(x, u as the kernel read it, the parameter table or None)``."""
    if x0.device.type != "cuda" or u.device != x0.device:
        raise RuntimeError(f"forging_rk4 runs on a ROCm device only (got x0 on {x0.device}, u on {u.device})")
    if x0.dim() != 2 or x0.shape[1] != 5:
        raise ValueError(f"x0 must be (B, 5), got {tuple(x0.shape)}")
    if u.dim() != 2 or u.shape[0] != x0.shape[0]:
        raise ValueError(f"u must be (B, S) with B = {x0.shape[0]}, got {tuple(u.shape)}")
    B, S = x0.shape[0], u.shape[1]
    x0c = x0.to(torch.float64).contiguous()
    uc = u.to(torch.float64).contiguous()
    out = torch.empty(B, S + 1, 5, dtype=torch.float64, device=x0.device)
    tab, name, extra = None, "fcr_plant_rk4", ()
    if params is not None:
        tab = as_press_table(params, x0.device)
        if tuple(tab.shape) not in ((28,), (B, 28)):
            raise ValueError(f"params must be a PressParams, (28,) or (B, 28) = {(B, 28)}, got {tuple(tab.shape)}")
        name, extra = "fcr_plant_rk4_press", (ctypes.c_void_p(tab.data_ptr()), 28 if tab.dim() == 2 else 0)
    _native.check(getattr(_native.load(), name)(B, S, float(ts), int(substeps), int(bool(smooth)),
                                                ctypes.c_void_p(x0c.data_ptr()), ctypes.c_void_p(uc.data_ptr()),
                                                ctypes.c_void_p(out.data_ptr()), *extra, _native.stream(x0.device)), name)
    return out, uc, tab


class _ForgingRK4Grad(torch.autograd.Function):
    """:func:`forging_rk4` attached to the graph: the forward is the plain launch, the backward ``fcr_plant_rk4_vjp`` on
    the stored states and commands (``fcr_plant_rk4_vjp_press`` when the parameter tensor asks for its gradient)."""

    @staticmethod
    def forward(ctx, x0, u, ts, substeps, smooth, params):
        x, uc, tab = _forging_rk4(x0, u, ts, substeps, smooth, params.detach() if torch.is_tensor(params) else params)
        ctx.save_for_backward(x, uc)
        ctx.tab, ctx.step, ctx.dtypes = tab, (ts, substeps, smooth), (x0.dtype, u.dtype)
        ctx.params_dtype = params.dtype if torch.is_tensor(params) else None
        return x

    @staticmethod
    def backward(ctx, g_x):
        x, uc = ctx.saved_tensors
        B, S = uc.shape
        ts, substeps, smooth = ctx.step
        g = g_x.to(torch.float64).contiguous()
        g_x0 = torch.empty(B, 5, dtype=torch.float64, device=x.device)
        g_u = torch.empty(B, S, dtype=torch.float64, device=x.device)
        tab = ctx.tab
        name, extra, g_params = "fcr_plant_rk4_vjp", (), None
        if ctx.needs_input_grad[5]:
            g_press = torch.empty(B, 28, dtype=torch.float64, device=x.device)
            name, extra = "fcr_plant_rk4_vjp_press", (ctypes.c_void_p(g_press.data_ptr()),)
        _native.check(getattr(_native.load(), name)(
            B, S, ts, substeps, int(smooth), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(uc.data_ptr()),
            ctypes.c_void_p(g.data_ptr()), None if tab is None else ctypes.c_void_p(tab.data_ptr()),
            28 if tab is not None and tab.dim() == 2 else 0, ctypes.c_void_p(g_x0.data_ptr()),
            ctypes.c_void_p(g_u.data_ptr()), *extra, _native.stream(x.device)), name)
        if extra:
            g_params = (g_press if tab.dim() == 2 else press_grad_sum(g_press)).to(ctx.params_dtype)
        return g_x0.to(ctx.dtypes[0]), g_u.to(ctx.dtypes[1]), None, None, None, g_params


class ForgingRK4:
    """Batched ``F(x0, u)`` of Functions.py:1743-1781: ``F(x0=(B,5), u=(B,))['xf'] -> (B, 5)``.

    Mirrors the CasADi Function's call convention (keyword inputs ``x0``, ``u``; output ``xf``) so the
    harness's ``F(x0=x, u=u)['xf']`` reads the same, for a batch of trajectories at once."""

    def __init__(self, TS: float = TS_REFERENCE, substeps: int = SUBSTEPS_REFERENCE, smooth: bool = False, params=None):
        self.TS, self.substeps, self.smooth, self.params = float(TS), int(substeps), bool(smooth), params

    def __call__(self, x0: torch.Tensor, u: torch.Tensor) -> dict:
        return {"xf": forging_rk4(x0, u.reshape(-1, 1), self.TS, self.substeps, self.smooth, self.params)[:, 1]}

    def rollout(self, x0: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
        """All S+1 states of the trajectories under commands u (B, S)."""
        return forging_rk4(x0, u, self.TS, self.substeps, self.smooth, self.params)


def fit_press(x_obs: torch.Tensor, u: torch.Tensor, fields, init: PressParams = PressParams(), ts: float = TS_REFERENCE,
              substeps: int = SUBSTEPS_REFERENCE, smooth: bool = False, max_iter: int = 60):
    """Fit ONE press, shared by all B trajectories, to recorded states ``x_obs (B, S+1, 5)`` under the recorded commands
    ``u (B, S)``: ``(PressParams, info)``.

    Single shooting from ``x_obs[:, 0]``: the unknowns are the log-multipliers q of the named ``fields`` (field =
    ``init``'s value times ``exp(q)``, so a :attr:`PressParams.POSITIVE` field stays positive; every other field keeps
    ``init``'s value), the loss is ``mean(((x - x_obs) / scale)^2)`` with ``x = forging_rk4(x_obs[:, 0], u, params=row)``
    and ``scale`` the per-state maximum of ``|x_obs|``, its gradient is :func:`forging_rk4`'s parameter gradient, and the
    optimiser is one ``step`` of ``torch.optim.LBFGS(lr=1, max_iter=max_iter, history_size=10,
    line_search_fn="strong_wolfe", tolerance_grad=1e-14, tolerance_change=1e-16)``. ``info``: ``loss0`` (at ``init``),
    ``loss`` (at the result), ``evals`` (loss + gradient evaluations) and ``multipliers`` (field -> ``exp(q)``).

    Which fields a trace can identify is the caller's business: a field the trace is insensitive to is NOT recovered —
    ``B_DAMP``, whose sensitivity on the reference's traces is three orders below ``CD``'s, ``M0``'s or ``KB``'s, stays
    where it started when fitted beside them — and fields that enter only through one coefficient (``CD`` and ``D``,
    ``M1`` and ``T_DEF``) cannot be told apart. Gradients through the press grow with S: a trace of
    hundreds of steps is the caller's risk; cut it into shorter ones. Runs on a ROCm device only."""
    fields = tuple(fields)
    unknown = [f for f in fields if f not in PressParams.NAMES]
    if unknown or not fields or len(set(fields)) != len(fields):
        raise ValueError(f"fit_press: fields must be distinct names of {PressParams.NAMES}, got {fields}")
    if not torch.is_tensor(x_obs) or not torch.is_tensor(u) or x_obs.device.type != "cuda" or u.device != x_obs.device:
        raise RuntimeError("fit_press runs on a ROCm device only (x_obs on "
                           f"{getattr(x_obs, 'device', 'the host')}, u on {getattr(u, 'device', 'the host')})")
    if u.dim() != 2 or x_obs.dim() != 3 or tuple(x_obs.shape) != (u.shape[0], u.shape[1] + 1, 5):
        raise ValueError(f"fit_press: x_obs must be (B, S+1, 5) and u (B, S); got {tuple(x_obs.shape)}, {tuple(u.shape)}")
    dev = x_obs.device
    x_obs, u = x_obs.detach().to(torch.float64), u.detach().to(torch.float64)
    x0 = x_obs[:, 0].contiguous()
    scale = x_obs.abs().amax((0, 1)).clamp_min(torch.finfo(torch.float64).tiny)
    base = torch.tensor(init.as_row(), dtype=torch.float64, device=dev)
    index = torch.tensor([PressParams.NAMES.index(f) for f in fields], device=dev)
    q = torch.zeros(len(fields), dtype=torch.float64, device=dev, requires_grad=True)

    def loss_of(q):
        row = base.index_put((index,), base[index] * torch.exp(q))
        x = forging_rk4(x0, u, ts, substeps, smooth, params=row)
        return (((x - x_obs) / scale) ** 2).mean()

    opt = torch.optim.LBFGS([q], lr=1, max_iter=int(max_iter), history_size=10, line_search_fn="strong_wolfe",
                            tolerance_grad=1e-14, tolerance_change=1e-16)
    evals = 0

    def closure():
        nonlocal evals
        evals += 1
        opt.zero_grad()
        loss = loss_of(q)
        loss.backward()
        return loss

    with torch.no_grad():
        loss0 = float(loss_of(q))
    opt.step(closure)
    with torch.no_grad():
        loss = float(loss_of(q))
        mult = torch.exp(q).cpu().tolist()
    fitted = init.replace(**{f: getattr(init, f) * m for f, m in zip(fields, mult)})
    return fitted, {"loss0": loss0, "loss": loss, "evals": evals, "multipliers": dict(zip(fields, mult))}
