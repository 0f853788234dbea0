"""Batched closed-loop evaluation on the GPU (SURVEY.md §8(f) ranks 1 + 2 together).

The reference evaluates its trained controller in ``NeuralNetwork.loop`` (Functions.py:1075-1240): for
each trajectory and step, the speed reference from ``tvp_fun`` (:926-966), the controller through
``FeasibilityRecovery.NN_make_step`` (:1560-1613, MaxAbs-scaled inputs, fp32 torch model, unscaled
output) and the press advanced by do-mpc's simulator — one trajectory at a time, in Python.
:class:`ClosedLoop` runs the controller and the press (the reference's RK4 integrator ``F`` of
``Ruge_Kuta``, Functions.py:1743-1781, on ``forging_model`` or the smooth ``template_model``) for a whole
batch of trajectories and all steps in ONE kernel launch (``fcr_closed_loop_run``,
forging-control_amd/csrc/fcr_closed_loop.h). do-mpc's process and measurement noise (``w0``, ``v0``,
Functions.py:1175-1183) are optional pre-drawn inputs of that launch: :func:`harness_noise` draws them in the
reference's order. :meth:`ClosedLoop.loop` adds the harness's second track, the LSTM surrogate stepped beside
the press on its own predictions and the controller's command (``results_LSTM``, Functions.py:1196-1231), as
one more launch (``fcr_lstm_rollout``, csrc/fcr_lstm_rollout.h). The reference's feasibility recovery
(``FeasibilityRecovery.feasibility_recover``, a CasADi/IPOPT solve per step) is :class:`FeasibilityRecovery`: its
NLP is the projection of one command onto the set that keeps both pressures inside their bounds over the next two
steps, which ``csrc/fcr_feasibility.h`` searches on the GPU, alone (``project``) or inside the loop's launch
(``feasibility=``).
"""
from __future__ import annotations

import ctypes
import random

import numpy as np
import torch

from . import _native
from .functions import _controller_params
from .inference import simulate_rollout
from .plant import SUBSTEPS_REFERENCE, TS_REFERENCE


def tvp_fun(t_now: float, ref_step: float, bias_work: int, bias_return: int, epsilon: float = 1e-7) -> float:
    """NeuralNetwork.tvp_fun (Functions.py:926-966): a random working-stroke speed in [0.1, 0.9] for the
    first half of every reference period and a random return-stroke speed in [-0.9, -0.1] for the second,
    each drawn from Python's generator seeded by the period index plus a bias."""
    phase = (t_now + epsilon) % ref_step
    period = (t_now + epsilon) // ref_step
    if phase < ref_step / 2:
        random.seed(period + bias_work)
        return 0.8 * random.random() + 0.1
    random.seed(period + bias_return)
    return -0.8 * random.random() - 0.1


def reference_speeds(n_traj: int, t_traj: int, ts: float, bias_work: int, bias_return: int) -> np.ndarray:
    """(n_traj, t_traj) references the harness uses: t_now = (idx·T_traj + t)·Ts, period Ts·T_traj
    (Functions.py:1116-1160)."""
    t_ref = ts * t_traj
    return np.array([[tvp_fun((i * t_traj + t) * ts, t_ref, bias_work, bias_return) for t in range(t_traj)]
                     for i in range(n_traj)])


def harness_noise(n_traj: int, t_traj: int, process_std, meas_std, rng: np.random.RandomState):
    """The harness's noise draws for a whole run, ``(w, v)`` each ``(n_traj, t_traj, 5)`` fp64, from ``rng`` in the
    reference's order (Functions.py:1176-1179, 1209-1210): trajectory by trajectory and step by step,
    ``normal(0, process_std)`` (5 values), ``normal(0, meas_std)`` (5), then the 4-value ``w0_NN`` draw, whose std is
    zero: it is discarded but consumes the stream, as does a zero std. (RandomState.normal is loc + scale * gauss over
    one sequential Gaussian stream, so the 14 draws of a step are one row of a single standard-normal block.)"""
    p = np.broadcast_to(np.asarray(process_std, np.float64), (5,))
    m = np.broadcast_to(np.asarray(meas_std, np.float64), (5,))
    if np.any(p < 0) or np.any(m < 0):
        raise ValueError("harness_noise: standard deviations must be >= 0")
    z = rng.standard_normal((int(n_traj), int(t_traj), 14))
    return 0.0 + p * z[..., 0:5], 0.0 + m * z[..., 5:10]


def _scale(s):
    """A MaxAbsScaler's ``scale_`` (sklearn object or plain number/array)."""
    return np.atleast_1d(np.asarray(getattr(s, "scale_", s), dtype=np.float64))


class FeasibilityRecovery:
    """The reference's feasibility recovery (UL/Main.py:584-657) as a projection on the GPU.

    The NLP has one scalar ``u``; its slacks are in the cost only, so it is ``min (u_nn - u)^2`` subject to
    ``p1`` and ``p2`` staying inside their bounds after one and two RK4 steps of the non-smooth ``forging_model``
    with ``u`` held. ``project(x (B,5), u_nn (B)) -> (u (B), flag (B) int32)``: flag 0 = ``u_nn`` is feasible and is
    returned bit for bit (also outside ``u_bounds``: the NLP does not bound ``u``); 1 = corrected to the nearest
    feasible command found by probing ``u_nn -/+ (u_hi - u_lo)/2^expand * 2^k`` (clipped to ``u_bounds``) for
    k = 0..expand and bisecting ``bisect`` times towards ``u_nn``; 2 = no probe is feasible and ``u`` is
    ``clip(u_nn, *u_bounds)``, the reference's ``except`` branch. The search returns the nearest feasible command
    wherever the feasible set is an interval on the probed side."""

    def __init__(self, p1=(0.0, 32e6), p2=(0.0, 32e6), u_bounds=(-0.2, 0.2), ts: float = TS_REFERENCE,
                 substeps: int = SUBSTEPS_REFERENCE, expand: int = 10, bisect: int = 30):
        self.p1, self.p2 = (float(p1[0]), float(p1[1])), (float(p2[0]), float(p2[1]))
        self.u_bounds = (float(u_bounds[0]), float(u_bounds[1]))
        self.ts, self.substeps, self.expand, self.bisect = float(ts), int(substeps), int(expand), int(bisect)

    def struct(self) -> _native.FcrFeasibility:
        return _native.FcrFeasibility(*self.p1, *self.p2, *self.u_bounds, self.ts, self.substeps, self.expand,
                                      self.bisect)

    def project(self, x: torch.Tensor, u_nn: torch.Tensor, return_violation: bool = False):
        """``return_violation``: also return ``v (B)``, the violation at the returned ``u`` (feasible iff <= 0)."""
        dev = x.device
        if dev.type != "cuda" or u_nn.device != dev:
            raise RuntimeError(f"FeasibilityRecovery runs on a ROCm device only (x on {x.device}, u_nn on {u_nn.device})")
        if x.dim() != 2 or x.shape[1] != 5 or u_nn.dim() != 1 or u_nn.shape[0] != x.shape[0]:
            raise ValueError(f"x must be (B,5) and u_nn (B,); got {tuple(x.shape)}, {tuple(u_nn.shape)}")
        B = x.shape[0]
        xc, uc = x.to(torch.float64).contiguous(), u_nn.to(torch.float64).contiguous()
        u = torch.empty(B, dtype=torch.float64, device=dev)
        flag = torch.empty(B, dtype=torch.int32, device=dev)
        v = torch.empty(B, dtype=torch.float64, device=dev) if return_violation else None
        f = self.struct()
        _native.check(_native.load().fcr_feasibility_project(
            ctypes.byref(f), B, xc.data_ptr(), uc.data_ptr(), u.data_ptr(), flag.data_ptr(),
            None if v is None else v.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
            "fcr_feasibility_project")
        return (u, flag, v) if return_violation else (u, flag)


class ClosedLoop:
    """Controller + press for B trajectories over T steps: ``run(x0 (B,5), ref (B,T))`` ->
    ``(x (B,T+1,5), u (B,T))`` as fp64 device tensors.

    ``scalers`` holds the controller's MaxAbs scalers as NN_make_step reads them: ``'input'`` (scale_ of
    [y_dot, z, ref]; the first two are used), ``'y_dot'`` (scales the reference) and ``'output'``."""

    def __init__(self, controller, scalers: dict, ts: float = TS_REFERENCE, substeps: int = SUBSTEPS_REFERENCE,
                 smooth: bool = True):
        self.controller = controller
        s_in = _scale(scalers["input"])
        self.in_scale = (float(s_in[0]), float(s_in[1]))
        self.ref_scale = float(_scale(scalers["y_dot"])[0])
        self.out_scale = float(_scale(scalers["output"])[0])
        self.ts, self.substeps, self.smooth = float(ts), int(substeps), bool(smooth)

    def run(self, x0: torch.Tensor, ref: torch.Tensor, process_noise: torch.Tensor | None = None,
            meas_noise: torch.Tensor | None = None, feasibility: FeasibilityRecovery | None = None):
        """``process_noise`` / ``meas_noise``: (B,T,5) pre-drawn ``w0`` / ``v0`` (:func:`harness_noise`), or None.
        ``w`` is in the units of x_dot and is held over the step: every RK4 stage evaluates f(x,u) + w[b,t].
        ``x[:,t+1]`` records x_{t+1} + v[b,t]; the controller reads that record, the press integrates on from the
        unperturbed state. (The smooth model measures p_eff, template_model.py:154-155; the record here is p + v.)
        Without noise the call returns exactly what it always did.

        ``feasibility``: a :class:`FeasibilityRecovery`; every step then projects the controller's command from the
        state the controller reads (under ``meas_noise`` the noisy record) and steps the press with the projected
        command. The call then returns ``(x, u, info)``: ``u`` the projected commands, ``info = {"u_nn": (B,T) the
        controller's raw commands, "flag": (B,T) int32 the projection's flags}``. With ``None`` it returns ``(x, u)``
        as it always did."""
        dev = x0.device
        if dev.type != "cuda" or ref.device != dev:
            raise RuntimeError(f"ClosedLoop runs on a ROCm device only (x0 on {x0.device}, ref on {ref.device})")
        if x0.dim() != 2 or x0.shape[1] != 5 or ref.dim() != 2 or ref.shape[0] != x0.shape[0]:
            raise ValueError(f"x0 must be (B,5) and ref (B,T); got {tuple(x0.shape)}, {tuple(ref.shape)}")
        B, T = x0.shape[0], ref.shape[1]
        noise = []
        for name, n in (("process_noise", process_noise), ("meas_noise", meas_noise)):
            if n is None:
                noise.append(None)
                continue
            if tuple(n.shape) != (B, T, 5):
                raise ValueError(f"{name} must be (B,T,5) = {(B, T, 5)}, got {tuple(n.shape)}")
            if n.device != dev:
                raise RuntimeError(f"{name} must be on {dev}, found it on {n.device}")
            noise.append(n.to(torch.float64).contiguous())
        W_inp, b_inp, W_out = (p.detach().to(device=dev, dtype=torch.float32).contiguous()
                               for p in _controller_params(self.controller))
        x0c = x0.to(torch.float64).contiguous()
        refc = ref.to(torch.float64).contiguous()
        x = torch.empty(B, T + 1, 5, dtype=torch.float64, device=dev)
        u = torch.empty(B, T, dtype=torch.float64, device=dev)
        p = lambda t: t.data_ptr()
        feas, info = (), None
        if feasibility is not None:
            info = {"u_nn": torch.empty(B, T, dtype=torch.float64, device=dev),
                    "flag": torch.empty(B, T, dtype=torch.int32, device=dev)}
            f_struct = feasibility.struct()                  # stays alive over the call below
            feas = (ctypes.pointer(f_struct), p(info["u_nn"]), p(info["flag"]))
        args = _native.FcrClosedLoop(B, T, self.ts, self.substeps, int(self.smooth), p(x0c), p(refc), p(W_inp),
                                     p(b_inp), p(W_out), W_inp.shape[0], (ctypes.c_double * 2)(*self.in_scale),
                                     self.ref_scale, self.out_scale, p(x), p(u),
                                     *(None if n is None else p(n) for n in noise), *feas)
        _native.check(_native.load().fcr_closed_loop_run(ctypes.byref(args),
                                                         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                      "fcr_closed_loop_run")
        return (x, u) if info is None else (x, u, info)

    def loop(self, x0: torch.Tensor, ref: torch.Tensor, simulator, model_scalers: dict,
             process_noise: torch.Tensor | None = None, meas_noise: torch.Tensor | None = None,
             lstm_noise: torch.Tensor | None = None, feasibility: FeasibilityRecovery | None = None):
        """``NeuralNetwork.loop``'s two tracks for B trajectories (Functions.py:1116-1273) in two launches: the press
        under the controller (:meth:`run`) and the LSTM surrogate free-running beside it on its own predictions and
        the press's commands (``inference.simulate_rollout`` on that run's ``u``).

        ``model_scalers``: the surrogate's MaxAbs scalers, ``'input'`` (scale_ of [y_dot, p1, p2, z, u]) and
        ``'output'`` (scale_ of [y_dot, p1, p2, z]). ``lstm_noise`` (B,T,4): the scaled ``w0_NN`` (the reference
        draws it with zero std). Returns ``(results, results_LSTM)``, dicts of fp64 device tensors keyed as the
        reference's (:1266-1273): ``results`` y, y_dot, p1, p2, z (B,T+1) and ref, u (B,T); ``results_LSTM`` y_dot,
        p1, p2, z (B,T+1), row 0 = x0[:,1:5]. With ``feasibility`` (:meth:`run`) ``results['u']`` holds the projected
        commands, which also drive the surrogate's track (Functions.py:1196), and ``results`` gains ``u_nn`` and
        ``feas_flag`` (B,T)."""
        x, u, *info = self.run(x0, ref, process_noise, meas_noise, feasibility)
        dev = x.device
        s_in, s_out = _scale(model_scalers["input"]), _scale(model_scalers["output"])
        if s_in.shape != (5,) or s_out.shape != (4,):
            raise ValueError(f"model_scalers: 'input' needs 5 scales and 'output' 4, got {s_in.shape[0]} and "
                             f"{s_out.shape[0]}")
        B, T = u.shape
        results = {"y": x[:, :, 0], "y_dot": x[:, :, 1], "p1": x[:, :, 2], "p2": x[:, :, 3], "z": x[:, :, 4],
                   "ref": ref.to(torch.float64), "u": u}
        if info:
            results["u_nn"], results["feas_flag"] = info[0]["u_nn"], info[0]["flag"]
        first = x[:, 0, 1:5]
        track = torch.empty(B, T + 1, 4, dtype=torch.float64, device=dev)
        track[:, 0] = first
        if T > 0:
            t_in = torch.tensor(s_in, dtype=torch.float64, device=dev)
            t_out = torch.tensor(s_out, dtype=torch.float64, device=dev)
            # the t = 0 window: [x0[1:5], u_0] scaled, repeated over the lookback rows (Functions.py:1196-1203)
            row0 = (torch.cat([first, u[:, :1]], dim=1) / t_in).to(torch.float32)
            window0 = row0[:, None, :].expand(B, 10, 5).contiguous()
            cmd = (u / t_in[4]).to(torch.float32)
            xhat = simulate_rollout(simulator, window0, cmd, gain=s_out / s_in[:4], noise=lstm_noise)
            track[:, 1:] = xhat.to(torch.float64) * t_out
        results_lstm = {"y_dot": track[:, :, 0], "p1": track[:, :, 1], "p2": track[:, :, 2], "z": track[:, :, 3]}
        return results, results_lstm
