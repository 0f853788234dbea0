"""The model-predictive baseline on the press: a shooting MPC with the reference's objective.

The reference compares every controller with a do-mpc/IPOPT MPC (``MPC.loop``, UL/Functions.py:1787-1943): horizon 10,
stage and terminal cost ``(y_dot - ref)^2``, ``rterm`` 0.02 on the command increments, optional pressure bounds.
:class:`PressMPC` solves that objective on the project's own RK4 press (:func:`~.plant.forging_rk4`'s step) for a batch
of trajectories, one GPU lane each, by a FIXED number of Levenberg-Marquardt iterations on the residuals (``fcr_mpc_solve``,
``fcr_mpc_closed_loop``; csrc/fcr_mpc.h). It is not the reference's transcription (collocation, interior point): commands
agree with the logged IPOPT ones where both are converged and differ in transients.

Residuals of one horizon from the state ``x_0`` with the previous command ``u_prev`` and references ``r_1..r_N``:
``e_k = x_k[1] - r_k`` (k = 1..N), ``d_k = sqrt(r_u) (u_k - u_{k-1})`` (k = 0..N-1, ``u_{-1} = u_prev``), and per pressure and
step the hinges ``sqrt(w) relu((p - hi)/s_p)``, ``sqrt(w) relu((lo - p)/s_p)``; ``cost = sum residual^2``. The hinges are
SQUARED in the cost, unlike :class:`~.loss_terms.LossTerms`' linear ones, because Gauss-Newton needs residuals. The command
box ``u_bounds`` is handled by an active set and clipping, the pressure bounds only softly (no hard state constraints).
"""
from __future__ import annotations

import ctypes

import torch

from . import _native
from .closed_loop import _LoopConfig
from .plant import SUBSTEPS_REFERENCE, TS_REFERENCE, as_press_table

INF = float("inf")


def _table(params, dev, B, what):
    """``params`` (None, PressParams, (28,) or (B,28)) -> (tensor or None, stride in elements)."""
    if params is None:
        return None, 0
    tab = as_press_table(params, dev, what)
    if tuple(tab.shape) not in ((28,), (B, 28)):
        raise ValueError(f"{what} must be a PressParams, (28,) or (B,28) with B = {B}, got shape {tuple(tab.shape)}")
    return tab, 28 if tab.dim() == 2 else 0


class PressMPC:
    """``PressMPC(n_horizon, iters, ...)``: the horizon N (1..32), the iterations K per solve (1..64), the weight ``r_u`` on
    command increments, the pressure bounds ``p1``, ``p2`` (Pa; infinite = off) with their weight ``p_weight`` (0 = off) and
    scale ``p_scale``, the command box ``u_bounds``, the initial damping ``lam0``, the integrator (``ts``, ``substeps``,
    ``smooth`` as :class:`~.closed_loop.ClosedLoop`) and ``model_params``: the press the controller's MODEL integrates — None
    (the reference's), a :class:`~.plant.PressParams` or ``(28,)`` row, or a ``(B,28)`` table, one row per trajectory."""

    def __init__(self, n_horizon: int = 10, iters: int = 3, r_u: float = 0.02, p1=(-INF, INF), p2=(-INF, INF),
                 p_weight: float = 0.0, p_scale: float = 32e6, u_bounds=(-INF, INF), lam0: float = 1e-3,
                 ts: float = TS_REFERENCE, substeps: int = SUBSTEPS_REFERENCE, smooth: bool = True, model_params=None):
        self.n_horizon, self.iters = int(n_horizon), int(iters)
        self.r_u, self.lam0, self.p_weight, self.p_scale = float(r_u), float(lam0), float(p_weight), float(p_scale)
        self.p1, self.p2 = (float(p1[0]), float(p1[1])), (float(p2[0]), float(p2[1]))
        self.u_bounds = (float(u_bounds[0]), float(u_bounds[1]))
        self.ts, self.substeps, self.smooth = float(ts), int(substeps), bool(smooth)
        self.model_params = model_params
        if not 1 <= self.n_horizon <= 32:
            raise ValueError(f"n_horizon = {n_horizon} must be 1..32")
        if not 1 <= self.iters <= 64:
            raise ValueError(f"iters = {iters} must be 1..64")
        if self.p1[0] > self.p1[1] or self.p2[0] > self.p2[1] or self.u_bounds[0] > self.u_bounds[1]:
            raise ValueError("a lower bound is above its upper bound")
        if not (self.r_u >= 0 and self.p_weight >= 0 and self.lam0 > 0 and self.p_scale > 0):
            raise ValueError("r_u and p_weight must be >= 0, lam0 and p_scale > 0")

    def struct(self) -> _native.FcrMpc:
        return _native.FcrMpc(self.n_horizon, self.iters, self.ts, self.substeps, int(self.smooth), self.r_u, self.lam0,
                              (ctypes.c_double * 4)(*self.p1, *self.p2), self.p_weight, self.p_scale,
                              (ctypes.c_double * 2)(*self.u_bounds))

    def _workspace(self, B, dev):
        size = ctypes.c_size_t(0)
        _native.check(_native.load().fcr_mpc_workspace_size(B, self.n_horizon, ctypes.byref(size)), "fcr_mpc_workspace_size")
        return torch.empty(max(size.value, 8), dtype=torch.uint8, device=dev)

    def solve(self, x0: torch.Tensor, ref: torch.Tensor, u_prev: torch.Tensor, U0: torch.Tensor | None = None,
              trace: bool = False) -> dict:
        """One horizon for B problems: ``x0 (B,5)``, ``ref (B,)`` (held over the horizon) or ``(B,N)``, ``u_prev (B,)``, the
        initial guess ``U0 (B,N)`` (default: ``u_prev`` repeated; projected into ``u_bounds``, so the returned ``U`` is inside
        the box even if no iteration is accepted, while ``u_prev`` is taken as given). Returns fp64 device tensors ``U (B,N)``, ``cost (B,)``,
        ``grad_inf (B,)`` (``|g|_inf`` over the non-active entries at the last point linearised), ``accepted (B,)`` int32,
        ``lam (B,)``; with ``trace=True`` also ``trace (B,K,5)`` — per iteration ``(c, c', lambda before, accepted, pivot
        failure)`` — and ``trace_U (B,K,N)``, U after each iteration."""
        dev, N, K = x0.device, self.n_horizon, self.iters
        if dev.type != "cuda":
            raise RuntimeError(f"PressMPC runs on a ROCm device only (x0 on {x0.device})")
        if x0.dim() != 2 or x0.shape[1] != 5:
            raise ValueError(f"x0 must be (B,5), got {tuple(x0.shape)}")
        B = x0.shape[0]
        if tuple(ref.shape) not in ((B,), (B, N)) or tuple(u_prev.shape) != (B,):
            raise ValueError(f"ref must be (B,) or (B,N) = {(B, N)} and u_prev (B,); got {tuple(ref.shape)}, {tuple(u_prev.shape)}")
        if U0 is not None and tuple(U0.shape) != (B, N):
            raise ValueError(f"U0 must be (B,N) = {(B, N)}, got {tuple(U0.shape)}")
        f64 = lambda t: None if t is None else t.detach().to(device=dev, dtype=torch.float64).contiguous()
        refc = f64(ref if ref.dim() == 2 else ref[:, None].expand(B, N))
        x0c, upc, U0c = f64(x0), f64(u_prev), f64(U0)
        tab, stride = _table(self.model_params, dev, B, "model_params")
        new = lambda *shape, dtype=torch.float64: torch.empty(*shape, dtype=dtype, device=dev)
        out = {"U": new(B, N), "cost": new(B), "grad_inf": new(B), "accepted": new(B, dtype=torch.int32), "lam": new(B)}
        if trace:
            out["trace"], out["trace_U"] = new(B, K, 5), new(B, K, N)
        ws = self._workspace(B, dev)
        p = lambda t: None if t is None else t.data_ptr()
        m = self.struct()
        _native.check(_native.load().fcr_mpc_solve(
            ctypes.byref(m), B, p(x0c), p(refc), p(upc), p(U0c), p(tab), stride, p(out["U"]), p(out["cost"]),
            p(out["grad_inf"]), p(out["accepted"]), p(out["lam"]), p(out.get("trace")), p(out.get("trace_U")), p(ws),
            ws.numel(), _native.stream(dev)), "fcr_mpc_solve")
        return out

    def run(self, x0: torch.Tensor, ref: torch.Tensor, process_noise: torch.Tensor | None = None,
            meas_noise: torch.Tensor | None = None, plant_params=None, preview: bool = True, u_init=0.0,
            U0: torch.Tensor | None = None, plans: bool = False, trace: bool = False) -> dict:
        """The closed loop of the MPC around the TRUE press for B trajectories over T steps in one launch: ``x0 (B,5)``,
        ``ref (B,T)``. Per step the controller reads the record ``x[:,t]`` (under ``meas_noise`` the noisy one, as
        :meth:`~.closed_loop.ClosedLoop.run` records it), solves from it with ``u_prev = u_{t-1}`` (``u_init`` at ``t = 0``: a
        number or ``(B,)``) warm-started from the previous plan shifted by one (``t = 0``: ``U0 (B,N)`` or ``u_init``
        repeated), applies ``U[0]`` and the press steps (``plant_params``: None, a row or ``(B,28)``; ``process_noise`` as
        the existing loop applies it). ``preview=True`` is the reference's ``tvp_fun`` behaviour, ``r_k = ref[min(t+k-1,
        T-1)]``; ``False`` holds ``ref[t]`` over the horizon.

        Returns ``x (B,T+1,5)``, ``u (B,T)``, each solve's ``cost``, ``grad_inf``, ``accepted`` ``(B,T)``; ``plans (B,T,N)``
        and ``trace (B,T,K,5)`` / ``trace_U (B,T,K,N)`` on request; and ``metrics``: :class:`~.closed_loop.ClosedLoopBank`'s
        figures over all B*T steps (``MAE``, ``RMSE``, ``R2``, ``max_err``, ``Command``, ``du_rms``, ``viol_max``,
        ``viol_frac`` against ``p1``/``p2``) as 0-dim fp64 tensors and ``traj`` — per trajectory ``MAE``, ``RMSE``, ``R2``,
        ``max_err``, ``Command``, ``du_rms``, ``viol_max`` ``(B,)`` — computed in torch from the record
        (:func:`loop_metrics`). A starting plan outside ``u_bounds`` is projected into the box, so every applied command
        is inside it; ``u_init`` as the previous command is taken as given."""
        dev, N, K = x0.device, self.n_horizon, self.iters
        if dev.type != "cuda" or ref.device != dev:
            raise RuntimeError(f"PressMPC runs on a ROCm device only (x0 on {x0.device}, ref on {ref.device})")
        if x0.dim() != 2 or x0.shape[1] != 5 or ref.dim() != 2 or ref.shape[0] != x0.shape[0]:
            raise ValueError(f"x0 must be (B,5) and ref (B,T); got {tuple(x0.shape)}, {tuple(ref.shape)}")
        B, T = ref.shape
        for name, n in (("process_noise", process_noise), ("meas_noise", meas_noise)):
            if n is not None and tuple(n.shape) != (B, T, 5):
                raise ValueError(f"{name} must be (B,T,5) = {(B, T, 5)}, got {tuple(n.shape)}")
        if U0 is not None and tuple(U0.shape) != (B, N):
            raise ValueError(f"U0 must be (B,N) = {(B, N)}, got {tuple(U0.shape)}")
        f64 = lambda t: None if t is None else t.detach().to(device=dev, dtype=torch.float64).contiguous()
        x0c, refc, wc, vc, U0c = f64(x0), f64(ref), f64(process_noise), f64(meas_noise), f64(U0)
        ui = f64(u_init) if torch.is_tensor(u_init) else torch.full((B,), float(u_init), dtype=torch.float64, device=dev)
        if tuple(ui.shape) != (B,):
            raise ValueError(f"u_init must be a number or (B,), got {tuple(ui.shape)}")
        ptab, pstride = _table(plant_params, dev, B, "plant_params")
        mtab, mstride = _table(self.model_params, dev, B, "model_params")
        new = lambda *shape, dtype=torch.float64: torch.empty(*shape, dtype=dtype, device=dev)
        out = {"x": new(B, T + 1, 5), "u": new(B, T), "cost": new(B, T), "grad_inf": new(B, T),
               "accepted": new(B, T, dtype=torch.int32)}
        if plans:
            out["plans"] = new(B, T, N)
        if trace:
            out["trace"], out["trace_U"] = new(B, T, K, 5), new(B, T, K, N)
        ws = self._workspace(B, dev)
        p = lambda t: None if t is None else t.data_ptr()
        m = self.struct()
        loop = _native.FcrMpcLoop(B, T, int(bool(preview)), p(x0c), p(refc), p(ui), p(U0c), p(wc), p(vc), p(ptab), pstride,
                                  p(mtab), mstride, p(out["x"]), p(out["u"]), p(out["cost"]), p(out["grad_inf"]),
                                  p(out["accepted"]), p(out.get("plans")), p(out.get("trace")), p(out.get("trace_U")))
        _native.check(_native.load().fcr_mpc_closed_loop(ctypes.byref(m), ctypes.byref(loop), p(ws), ws.numel(),
                                                         _native.stream(dev)), "fcr_mpc_closed_loop")
        out["ref"] = refc
        out["metrics"] = loop_metrics(out["x"], out["u"], refc, self.p1, self.p2)
        return out


def loop_metrics(x: torch.Tensor, u: torch.Tensor, ref: torch.Tensor, p1=(0.0, 32e6), p2=(0.0, 32e6)) -> dict:
    """:class:`~.closed_loop.ClosedLoopBank`'s figures from a record ``x (B,T+1,5)``, ``u (B,T)``, ``ref (B,T)`` in torch:
    with ``e = x[:,t+1,1] - ref[:,t]``, ``MAE``, ``RMSE``, ``R2 = 1 - SSE/SST`` (SST about the mean reference; SST = 0 gives
    1 or 0 as sklearn), ``max_err``, ``Command`` (mean ``|u|``), ``du_rms`` over the B (T-1) increments, ``viol_max`` = the
    worst of ``lo - p``, ``p - hi`` over the records' pressures (Pa) and ``viol_frac``, the share of steps with a positive
    one (with all four bounds infinite, the default, nothing can be violated: ``viol_max`` is ``-inf`` and ``viol_frac`` 0);
    ``traj``: the per-trajectory ``MAE``, ``RMSE``, ``R2`` (SST about the trajectory's own mean reference), ``max_err``,
    ``Command``, ``du_rms``, ``viol_max`` ``(B,)``. Empty runs give zeros."""
    B, T = u.shape
    z = torch.zeros((), dtype=torch.float64, device=u.device)
    if B == 0 or T == 0:
        zb = torch.zeros(B, dtype=torch.float64, device=u.device)
        return {**{k: z for k in ("MAE", "RMSE", "R2", "max_err", "Command", "du_rms", "viol_max", "viol_frac")},
                "traj": {k: zb for k in ("MAE", "RMSE", "R2", "max_err", "Command", "du_rms", "viol_max")}}
    e = x[:, 1:, 1] - ref
    sse, sst = (e * e).sum(), ((ref - ref.mean()) ** 2).sum()
    r2 = torch.where(sst > 0, 1 - sse / torch.where(sst > 0, sst, torch.ones_like(sst)), (sse == 0).to(torch.float64))
    du = u[:, 1:] - u[:, :-1]
    pa, pb = x[:, 1:, 2], x[:, 1:, 3]
    viol = torch.stack([p1[0] - pa, pa - p1[1], p2[0] - pb, pb - p2[1]]).amax(0)
    ones = lambda t: torch.where(t > 0, t, torch.ones_like(t))
    sse_b, sst_b = (e * e).sum(1), ((ref - ref.mean(1, keepdim=True)) ** 2).sum(1)
    traj = {"MAE": e.abs().mean(1), "RMSE": (e * e).mean(1).sqrt(),
            "R2": torch.where(sst_b > 0, 1 - sse_b / ones(sst_b), (sse_b == 0).to(torch.float64)),
            "max_err": e.abs().amax(1), "Command": u.abs().mean(1),
            "du_rms": (du * du).mean(1).sqrt() if T > 1 else torch.zeros_like(u[:, 0]), "viol_max": viol.amax(1)}
    return {"MAE": e.abs().mean(), "RMSE": (e * e).mean().sqrt(), "R2": r2, "max_err": e.abs().max(),
            "Command": u.abs().mean(), "du_rms": (du * du).mean().sqrt() if T > 1 else z, "viol_max": viol.max(),
            "viol_frac": (viol > 0).to(torch.float64).mean(), "traj": traj}


def mpc_dataset(result: dict, scalers):
    """The supervised table of an MPC run: ``X (B*T,3)`` = the controller's scaled inputs ``(y_dot, z, ref)`` at each step's
    record and ``y (B*T,1)`` = the MPC's scaled command, float32 on the run's device, as ``supervised.train_epoch`` takes
    them. ``scalers``: the controller's MaxAbs scalers as :class:`~.closed_loop.ClosedLoop` reads them (``'input'``: the
    first two scales; ``'y_dot'`` scales the reference; ``'output'`` the command)."""
    s = _LoopConfig(scalers, TS_REFERENCE, SUBSTEPS_REFERENCE, True)
    x, u, ref = result["x"], result["u"], result["ref"]
    X = torch.stack([x[:, :-1, 1] / s.in_scale[0], x[:, :-1, 4] / s.in_scale[1], ref / s.ref_scale], -1)
    return X.reshape(-1, 3).to(torch.float32), (u / s.out_scale).reshape(-1, 1).to(torch.float32)
