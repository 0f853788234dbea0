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
(``feasibility=``). :class:`ClosedLoopBank` runs the M controllers of a ``ControllerBank`` through that loop in one
launch (``fcr_closed_loop_run_bank``) and returns the evaluation's numbers — the reference's ``metrics`` /
``other_metrics`` (Functions.py:751-822), command smoothness and constraint violation — accumulated in the loop kernel.
"""
from __future__ import annotations

import ctypes
import random
import types

import numpy as np
import torch

from . import _native
from .functions import _controller_params
from .inference import simulate_rollout
from .plant import SUBSTEPS_REFERENCE, TS_REFERENCE, PressParams, as_press_table, press_grad_sum


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
    wherever the feasible set is an interval on the probed side.

    ``model_params``: the press the projection's MODEL integrates — a :class:`~.plant.PressParams` or a ``(28,)`` row,
    one set per call; ``None`` is the reference's press, the projection as it always was. Inside a loop it is the
    controller's idea of the press and need not be the press the loop steps (``plant_params`` there)."""

    def __init__(self, p1=(0.0, 32e6), p2=(0.0, 32e6), u_bounds=(-0.2, 0.2), ts: float = TS_REFERENCE,
                 substeps: int = SUBSTEPS_REFERENCE, expand: int = 10, bisect: int = 30, model_params=None):
        if model_params is not None and not isinstance(model_params, PressParams):
            row = np.asarray(torch.as_tensor(model_params).cpu(), dtype=np.float64)
            if row.shape != (28,):
                raise ValueError(f"model_params must be a PressParams or a (28,) row, got shape {row.shape}")
            model_params = PressParams(*row.tolist())
        self.model_params = model_params
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
        name, extra = "fcr_feasibility_project", ()
        if self.model_params is not None:
            model = self.model_params.struct()               # stays alive over the call below
            name, extra = "fcr_feasibility_project_press", (ctypes.byref(model),)
        _native.check(getattr(_native.load(), name)(
            ctypes.byref(f), *extra, B, xc.data_ptr(), uc.data_ptr(), u.data_ptr(), flag.data_ptr(),
            None if v is None else v.data_ptr(), _native.stream(dev)), name)
        return (u, flag, v) if return_violation else (u, flag)


def _per_model(name, t, M, tail):
    """Whether ``t`` is ``(M,) + tail`` (True) or ``tail``, one copy shared by all models (False); ``M = None``: the
    single loop, ``tail`` alone."""
    if tuple(t.shape) == tail:
        return False
    if M is not None and tuple(t.shape) == (M,) + tail:
        return True
    forms = f"(B,T,{tail[-1]}) = {tail}" if M is None else f"{tail} (shared by all models) or {(M,) + tail}"
    raise ValueError(f"{name} must be {forms}, got {tuple(t.shape)}")


class _LoopConfig:
    """What :class:`ClosedLoop` and :class:`ClosedLoopBank` hold alike — the controller's scales as the kernels take
    them, ``ts``, ``substeps``, ``smooth`` — and how both turn a run's inputs into the arguments of its launch."""

    def __init__(self, scalers, ts, substeps, smooth):
        if isinstance(scalers, _LoopConfig):                 # another loop's scales, as they are
            self.in_scale, self.ref_scale, self.out_scale = scalers.in_scale, scalers.ref_scale, scalers.out_scale
        else:
            s_in = _scale(scalers["input"])
            self.in_scale = (float(s_in[0]), float(s_in[1]))
            self.ref_scale = float(_scale(scalers["y_dot"])[0])
            self.out_scale = float(_scale(scalers["output"])[0])
        self.ts, self.substeps, self.smooth = float(ts), int(substeps), bool(smooth)

    def _prepare(self, M, weights, x0, ref, process_noise, meas_noise, feasibility, store=True):
        """The checks and conversions of a run: ``M = None`` for one model (inputs without a leading M), else the bank's M.
        Returns ``(dev, B, T, stacked, out, prefix, keep)``: which inputs carry a leading M, the per-step outputs
        (``x, u, u_nn, flag``; ``None`` where not stored), the constructor arguments of ``FcrClosedLoop`` (the fields
        ``FcrClosedLoopBank`` begins with), and what must stay alive over the call."""
        who, dev = type(self).__name__, x0.device
        noises = {"process_noise": process_noise, "meas_noise": meas_noise}

        def on_device():
            if dev.type != "cuda" or ref.device != dev:
                raise RuntimeError(f"{who} runs on a ROCm device only (x0 on {x0.device}, ref on {ref.device})")

        if M is None:
            on_device()                                      # one model: the device first; the bank: the shapes first
        dims = (2,) if M is None else (2, 3)
        if x0.dim() not in dims or x0.shape[-1] != 5 or ref.dim() not in dims or (M is None and ref.shape[0] != x0.shape[0]):
            forms = "(B,5) and ref (B,T)" if M is None else "(B,5) or (M,B,5) and ref (B,T) or (M,B,T)"
            raise ValueError(f"x0 must be {forms}; got {tuple(x0.shape)}, {tuple(ref.shape)}")
        B, T = x0.shape[-2], ref.shape[-1]
        stacked = {"x0": _per_model("x0", x0, M, (B, 5)), "ref": _per_model("ref", ref, M, (B, T))}
        for name, n in noises.items():
            stacked[name] = n is not None and _per_model(name, n, M, (B, T, 5))
        if M is not None:
            on_device()
        for name, n in noises.items():
            if n is not None and n.device != dev:
                raise RuntimeError(f"{name} must be on {dev}, found it on {n.device}")
        f64 = lambda t: None if t is None else t.to(torch.float64).contiguous()
        x0c, refc, wc, vc = f64(x0), f64(ref), f64(process_noise), f64(meas_noise)
        W_inp, b_inp, W_out = (p.detach().to(device=dev, dtype=torch.float32).contiguous() for p in weights)
        lead = () if M is None else (M,)
        new = lambda *shape, dtype=torch.float64: torch.empty(*lead, *shape, dtype=dtype, device=dev) if store else None
        out = {"x": new(B, T + 1, 5), "u": new(B, T), "u_nn": None, "flag": None}
        f_struct = None
        if feasibility is not None:
            f_struct = feasibility.struct()
            out["u_nn"], out["flag"] = new(B, T), new(B, T, dtype=torch.int32)
        p = lambda t: None if t is None else t.data_ptr()
        prefix = (B, T, self.ts, self.substeps, int(self.smooth), p(x0c), p(refc), p(W_inp), p(b_inp), p(W_out),
                  W_inp.shape[-2], (ctypes.c_double * 2)(*self.in_scale), self.ref_scale, self.out_scale, p(out["x"]),
                  p(out["u"]), p(wc), p(vc), None if f_struct is None else ctypes.pointer(f_struct), p(out["u_nn"]),
                  p(out["flag"]))
        return dev, B, T, stacked, out, prefix, (x0c, refc, wc, vc, W_inp, b_inp, W_out, f_struct)


class ClosedLoop(_LoopConfig):
    """Controller + press for B trajectories over T steps: ``run(x0 (B,5), ref (B,T))`` ->
    ``(x (B,T+1,5), u (B,T))`` as fp64 device tensors.

    ``scalers`` holds the controller's MaxAbs scalers as NN_make_step reads them: ``'input'`` (scale_ of
    [y_dot, z, ref]; the first two are used), ``'y_dot'`` (scales the reference) and ``'output'``."""

    def __init__(self, controller, scalers: dict, ts: float = TS_REFERENCE, substeps: int = SUBSTEPS_REFERENCE,
                 smooth: bool = True, plant_params=None):
        super().__init__(scalers, ts, substeps, smooth)
        self.controller = controller
        self.plant_params = plant_params                     # the default of run(plant_params=...)

    def run(self, x0: torch.Tensor, ref: torch.Tensor, process_noise: torch.Tensor | None = None,
            meas_noise: torch.Tensor | None = None, feasibility: FeasibilityRecovery | None = None, plant_params=None,
            differentiable: bool = False):
        """``process_noise`` / ``meas_noise``: (B,T,5) pre-drawn ``w0`` / ``v0`` (:func:`harness_noise`), or None.
        ``w`` is in the units of x_dot and is held over the step: every RK4 stage evaluates f(x,u) + w[b,t].
        ``x[:,t+1]`` records x_{t+1} + v[b,t]; the controller reads that record, the press integrates on from the
        unperturbed state. (The smooth model measures p_eff, template_model.py:154-155; the record here is p + v.)
        Without noise the call returns exactly what it always did.

        ``feasibility``: a :class:`FeasibilityRecovery`; every step then projects the controller's command from the
        state the controller reads (under ``meas_noise`` the noisy record) and steps the press with the projected
        command. The call then returns ``(x, u, info)``: ``u`` the projected commands, ``info = {"u_nn": (B,T) the
        controller's raw commands, "flag": (B,T) int32 the projection's flags}``. With ``None`` it returns ``(x, u)``
        as it always did.

        ``plant_params``: the press the loop steps — a :class:`~.plant.PressParams` or ``(28,)`` row for all
        trajectories, or a ``(B,28)`` table, one row per trajectory; ``None``: the constructor's, by default the
        reference's press. With parameters (here or as the ``feasibility``'s ``model_params``) the call runs the bank's
        kernels with one model (:class:`ClosedLoopBank`), whose trajectories are this loop's bit for bit.

        ``differentiable=True``: ``(x, u)`` are attached to the graph of the controller's three parameters and of ``x0``
        (under ``torch.no_grad()`` they come back detached). The forward is the launch above, ``x`` and ``u`` bit-equal to
        ``differentiable=False``; the backward is the adjoint of the loop (``fcr_closed_loop_vjp``, csrc/fcr_press_grad.h;
        DESIGN.md §7.13) on the stored ``x, u``, with ``plant_params`` in every form above; gradients reach the parameters
        in their own dtype, summed in fp64 in a fixed order (two backward calls give the same bits). The fp32 controller
        chain is recomputed in the forward's operation order, so its ReLU masks (ReLU'(0) = 0) and Hardtanh mask (1 only
        for ``-1 < v < 1``) are the forward's own; float casts count as the identity. The press's conventions where its
        derivative is singular are :func:`~.plant.forging_rk4`'s: deformation force differentiated only where ``y > 0``
        and ``y_dot > 0``; valve-flow derivatives 0 at a zero pressure difference, branch by ``z >= 0``; friction slope
        ``FT/0.5`` where ``|y_dot| <= 0.5``, else 0; smooth floor ``0.5 (1 + p / sqrt(p^2 + eps))``. Raises ``ValueError``
        with ``process_noise``, ``meas_noise`` (the record ``x + v`` does not give the unperturbed state back exactly:
        :meth:`run_differentiable` stores it and is the call under noise) or ``feasibility`` (the projection is not
        differentiable). No gradient reaches ``ref``. Gradients through the press
        grow with T: back-propagation through hundreds of steps is the caller's risk.

        Gradients reach the press too: a ``plant_params`` tensor, ``(28,)`` or ``(B,28)``, that requires
        grad is part of the graph (``fcr_closed_loop_vjp_press``); its ``.grad`` has its shape, dtype and device, for a
        ``(28,)`` row the fixed-order fp64 sum over the trajectories. The parameters follow the same conventions: the
        deformation fields (``MU, K, W0, H0, B0, T_DEF, M0..M4``) receive gradient only where ``y > 0`` and ``y_dot > 0``;
        ``CD, RHO, D, PS, PT`` receive 0 from a valve at a zero pressure difference, ``PS`` and ``PT`` by the branch
        ``z >= 0``; ``FT`` receives ``y_dot / 0.5`` inside the knee and 1 outside. A :class:`~.plant.PressParams` is a
        constant. :class:`ClosedLoopBank` has its own adjoint for M models in one launch, without the press's gradients
        (``ClosedLoopBank.run(differentiable=True)``)."""
        if plant_params is None:
            plant_params = self.plant_params
        if differentiable:
            for name, given in (("process_noise", process_noise), ("meas_noise", meas_noise), ("feasibility", feasibility)):
                if given is not None:
                    raise ValueError(f"ClosedLoop.run(differentiable=True) does not take {name}: the adjoint covers the "
                                     "noise-free loop without recovery (DESIGN.md §7.13); under noise: run_differentiable "
                                     "(§7.18)")
            if torch.is_grad_enabled():
                return _ClosedLoopGrad.apply(self, x0, ref, plant_params, *_controller_params(self.controller))
        if plant_params is not None or (feasibility is not None and feasibility.model_params is not None):
            if x0.dim() != 2 or ref.dim() != 2:
                raise ValueError(f"x0 must be (B,5) and ref (B,T); got {tuple(x0.shape)}, {tuple(ref.shape)}")
            if plant_params is not None and _press_shape(plant_params) not in ((28,), (x0.shape[0], 28)):
                raise ValueError(f"plant_params must be a PressParams, (28,) or (B,28) with B = {x0.shape[0]}, got shape "
                                 f"{_press_shape(plant_params)}")
            one = ClosedLoopBank.of_loop(self)
            r = one.run(x0, ref, process_noise, meas_noise, feasibility, plant_params=plant_params)
            if feasibility is None:
                return r["x"][0], r["u"][0]
            return r["x"][0], r["u"][0], {"u_nn": r["u_nn"][0], "flag": r["flag"][0]}
        dev, _, _, _, out, prefix, keep = self._prepare(None, _controller_params(self.controller), x0, ref, process_noise,
                                                        meas_noise, feasibility)
        args = _native.FcrClosedLoop(*prefix)
        _native.check(_native.load().fcr_closed_loop_run(ctypes.byref(args), _native.stream(dev)), "fcr_closed_loop_run")
        if feasibility is None:
            return out["x"], out["u"]
        return out["x"], out["u"], {"u_nn": out["u_nn"], "flag": out["flag"]}

    def run_differentiable(self, x0: torch.Tensor, ref: torch.Tensor, process_noise: torch.Tensor | None = None,
                           meas_noise: torch.Tensor | None = None, plant_params=None, truncate: int = 0, p_bounds=None):
        """:meth:`ClosedLoopBank.run_differentiable` for this loop as a bank of one: ``x0 (B,5)``,
        ``ref (B,T)``, each noise ``(B,T,5)`` or ``None``, ``plant_params`` as :meth:`run` takes it (a constant here).
        Returns the bank's dict with ``x (B,T+1,5)`` and ``u (B,T)`` attached to the controller's parameters and to
        ``x0``, and the detached ``x_state (B,T+1,5)``, each without the model dimension; every other entry is the bank
        of one's (leading dimension 1)."""
        if plant_params is None:
            plant_params = self.plant_params
        if x0.dim() != 2 or ref.dim() != 2:
            raise ValueError(f"x0 must be (B,5) and ref (B,T); got {tuple(x0.shape)}, {tuple(ref.shape)}")
        if plant_params is not None and _press_shape(plant_params) not in ((28,), (x0.shape[0], 28)):
            raise ValueError(f"plant_params must be a PressParams, (28,) or (B,28) with B = {x0.shape[0]}, got shape "
                             f"{_press_shape(plant_params)}")
        w_inp, b_inp, w_out = _controller_params(self.controller)
        out = ClosedLoopBank.of_loop(self).run_differentiable(
            x0, ref, process_noise, meas_noise, plant_params, truncate, p_bounds,
            _weights=(w_inp[None], b_inp[None], w_out.reshape(1, -1)))
        return {**out, "x": out["x"][0], "u": out["u"][0], "x_state": out["x_state"][0]}

    def loop(self, x0: torch.Tensor, ref: torch.Tensor, simulator, model_scalers: dict,
             process_noise: torch.Tensor | None = None, meas_noise: torch.Tensor | None = None,
             lstm_noise: torch.Tensor | None = None, feasibility: FeasibilityRecovery | None = None, plant_params=None):
        """``NeuralNetwork.loop``'s two tracks for B trajectories (Functions.py:1116-1273) in two launches: the press
        under the controller (:meth:`run`) and the LSTM surrogate free-running beside it on its own predictions and
        the press's commands (``inference.simulate_rollout`` on that run's ``u``).

        ``model_scalers``: the surrogate's MaxAbs scalers, ``'input'`` (scale_ of [y_dot, p1, p2, z, u]) and
        ``'output'`` (scale_ of [y_dot, p1, p2, z]). ``lstm_noise`` (B,T,4): the scaled ``w0_NN`` (the reference
        draws it with zero std). Returns ``(results, results_LSTM)``, dicts of fp64 device tensors keyed as the
        reference's (:1266-1273): ``results`` y, y_dot, p1, p2, z (B,T+1) and ref, u (B,T); ``results_LSTM`` y_dot,
        p1, p2, z (B,T+1), row 0 = x0[:,1:5]. With ``feasibility`` (:meth:`run`) ``results['u']`` holds the projected
        commands, which also drive the surrogate's track (Functions.py:1196), and ``results`` gains ``u_nn`` and
        ``feas_flag`` (B,T). ``plant_params`` (:meth:`run`) is the press's own; the surrogate was trained on the reference's
        press and its track is what it was."""
        x, u, *info = self.run(x0, ref, process_noise, meas_noise, feasibility, plant_params=plant_params)
        s_in, s_out = _model_scales(model_scalers)
        results = {"y": x[:, :, 0], "y_dot": x[:, :, 1], "p1": x[:, :, 2], "p2": x[:, :, 3], "z": x[:, :, 4],
                   "ref": ref.to(torch.float64), "u": u}
        if info:
            results["u_nn"], results["feas_flag"] = info[0]["u_nn"], info[0]["flag"]
        track = _shadow_track(x[:, 0, 1:5], u, simulator, s_in, s_out, lstm_noise)
        results_lstm = {"y_dot": track[:, :, 0], "p1": track[:, :, 1], "p2": track[:, :, 2], "z": track[:, :, 3]}
        return results, results_lstm


class _ClosedLoopGrad(torch.autograd.Function):
    """:meth:`ClosedLoop.run` attached to the graph: the forward is the plain launch (which reads the controller's
    parameters itself), the backward ``fcr_closed_loop_vjp`` on the stored run."""

    @staticmethod
    def forward(ctx, loop, x0, ref, plant_params, w_inp, b_inp, w_out):
        if torch.is_tensor(plant_params):
            plant_params = plant_params.detach()
        x, u = loop.run(x0, ref, plant_params=plant_params)
        dev = x.device
        ctx.loop = loop
        ctx.tab = None if plant_params is None else as_press_table(plant_params, dev, "plant_params")
        ctx.press_like = (plant_params.shape, plant_params.dtype) if torch.is_tensor(plant_params) else None
        ctx.like = tuple((t.shape, t.device, t.dtype) for t in (x0, w_inp, b_inp, w_out))
        ctx.save_for_backward(x, u, ref.to(torch.float64).contiguous(),
                              *(p.detach().to(device=dev, dtype=torch.float32).contiguous() for p in (w_inp, b_inp, w_out)))
        return x, u

    @staticmethod
    def backward(ctx, g_x, g_u):
        x, u, ref, w_inp, b_inp, w_out = ctx.saved_tensors
        press_grad = ctx.needs_input_grad[3]
        g = loop_vjp(ctx.loop, x, u, ref, g_x, g_u, (w_inp, b_inp, w_out), ctx.tab, press_grad=press_grad)
        like = lambda t, to: t.reshape(to[0]).to(device=to[1], dtype=to[2])
        x0_, wi_, bi_, wo_ = ctx.like
        g_params = g["g_press"].reshape(ctx.press_like[0]).to(ctx.press_like[1]) if press_grad else None
        return (None, like(g["g_x0"], x0_), None, g_params, like(g["g_w_inp"], wi_), like(g["g_b_inp"], bi_),
                like(g["g_w_out"], wo_))


def loop_vjp(loop: "ClosedLoop", x: torch.Tensor, u: torch.Tensor, ref: torch.Tensor, g_x: torch.Tensor, g_u: torch.Tensor,
             weights=None, plant_params=None, press_grad: bool = False) -> dict:
    """The vector-Jacobian product of a noise-free :meth:`ClosedLoop.run` without recovery (``fcr_closed_loop_vjp``): from
    the stored ``x (B,T+1,5)``, ``u (B,T)``, the ``ref`` of that run and the incoming ``g_x``, ``g_u``, a dict of fp64
    tensors ``g_x0 (B,5)``, ``dv (B,T)`` (the gradient at the controller's clamped fp32 output), ``g_w_inp (H,3)``,
    ``g_b_inp (H)``, ``g_w_out (H)``. ``weights``: the controller's three parameters as the run read them (default:
    ``loop.controller``'s now); ``plant_params``: the run's. ``press_grad=True`` (``fcr_closed_loop_vjp_press``) adds
    ``g_press``, the gradient of the press's 28 fields in ``plant_params``' shape: ``(B,28)`` for a table, for one row
    (a ``(28,)`` tensor, a :class:`~.plant.PressParams`, or ``None``: the reference's press) ``(28,)``, the fixed-order sum
    over the trajectories. This is what ``run(differentiable=True)`` calls in its backward; conventions: there."""
    dev = x.device
    if dev.type != "cuda":
        raise RuntimeError(f"ClosedLoop runs on a ROCm device only (x on {x.device})")
    B, T = u.shape
    if tuple(x.shape) != (B, T + 1, 5) or tuple(ref.shape) != (B, T) or tuple(g_x.shape) != (B, T + 1, 5) or \
            tuple(g_u.shape) != (B, T):
        raise ValueError(f"loop_vjp: x, g_x must be (B,T+1,5) and u, ref, g_u (B,T); got {tuple(x.shape)}, {tuple(g_x.shape)}, "
                         f"{tuple(u.shape)}, {tuple(ref.shape)}, {tuple(g_u.shape)}")
    f64 = lambda t: t.to(device=dev, dtype=torch.float64).contiguous()
    x, u, ref, gx, gu = f64(x), f64(u), f64(ref), f64(g_x), f64(g_u)
    w_inp, b_inp, w_out = (t.detach().to(device=dev, dtype=torch.float32).contiguous()
                           for t in (_controller_params(loop.controller) if weights is None else weights))
    if plant_params is None and press_grad:
        plant_params = PressParams()
    tab = None if plant_params is None else as_press_table(plant_params, dev, "plant_params")
    if tab is not None and tuple(tab.shape) not in ((28,), (B, 28)):
        raise ValueError(f"plant_params must be a PressParams, (28,) or (B,28) with B = {B}, got shape {tuple(tab.shape)}")
    H = w_inp.shape[0]
    new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)
    out = {"g_x0": new(B, 5), "dv": new(B, T), "g_w_inp": new(H, 3), "g_b_inp": new(H), "g_w_out": new(H)}
    lib = _native.load()
    size = ctypes.c_size_t(0)
    _native.check(lib.fcr_closed_loop_vjp_workspace_size(B, T, H, ctypes.byref(size)), "fcr_closed_loop_vjp_workspace_size")
    ws = torch.empty(max(size.value, 8), dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()
    args = _native.FcrClosedLoopGrad(
        B, T, loop.ts, loop.substeps, int(loop.smooth), p(ref), p(w_inp), p(b_inp), p(w_out), H,
        (ctypes.c_double * 2)(*loop.in_scale), loop.ref_scale, loop.out_scale, p(x), p(u), p(gx), p(gu),
        None if tab is None else p(tab), 28 if tab is not None and tab.dim() == 2 else 0,
        p(out["g_x0"]), p(out["dv"]), p(out["g_w_inp"]), p(out["g_b_inp"]), p(out["g_w_out"]))
    if press_grad:
        g_press = new(B, 28)
        _native.check(lib.fcr_closed_loop_vjp_press(ctypes.byref(args), ctypes.c_void_p(p(g_press)), ctypes.c_void_p(p(ws)),
                                                    ws.numel(), _native.stream(dev)), "fcr_closed_loop_vjp_press")
        out["g_press"] = g_press if tab.dim() == 2 else press_grad_sum(g_press)
        return out
    _native.check(lib.fcr_closed_loop_vjp(ctypes.byref(args), ctypes.c_void_p(p(ws)), ws.numel(), _native.stream(dev)),
                  "fcr_closed_loop_vjp")
    return out


def _press_shape(params) -> tuple:
    """The shape of ``plant_params`` (a PressParams is one row), without moving or converting it."""
    return (28,) if isinstance(params, PressParams) else tuple(np.shape(params))


def _model_scales(model_scalers: dict):
    s_in, s_out = _scale(model_scalers["input"]), _scale(model_scalers["output"])
    if s_in.shape != (5,) or s_out.shape != (4,):
        raise ValueError(f"model_scalers: 'input' needs 5 scales and 'output' 4, got {s_in.shape[0]} and "
                         f"{s_out.shape[0]}")
    return s_in, s_out


def _shadow_track(first: torch.Tensor, u: torch.Tensor, simulator, s_in, s_out, lstm_noise):
    """The surrogate's track (Functions.py:1196-1231) for R rows: ``first (R,4)`` = x0[:,1:5], ``u (R,T)`` the applied
    commands -> ``(R,T+1,4)`` fp64, row 0 = ``first``; one ``simulate_rollout`` launch."""
    dev = u.device
    B, T = u.shape
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
    return track


METRIC_KEYS = ("MAE", "RMSE", "R2", "max_err", "Command", "du_rms", "viol_max", "viol_frac", "flag1_frac", "flag2_frac")


class ClosedLoopBank(_LoopConfig):
    """:class:`ClosedLoop` for the M controllers of a :class:`~.many.ControllerBank` (one hidden width, one set of
    scalers): M x B trajectories over T steps in ONE launch (``fcr_closed_loop_run_bank``), and the numbers the
    reference tabulates per seed (``metrics`` / ``other_metrics``, Functions.py:751-822) from the same launch plus one
    small reduction. Model m's trajectories are ``ClosedLoop(controller_m).run(...)``'s on model m's inputs, bit for bit.

    ``run`` returns a dict:

    * ``x (M,B,T+1,5)``, ``u (M,B,T)`` and, under ``feasibility``, ``u_nn (M,B,T)``, ``flag (M,B,T)`` int32 — or ``None``
      each with ``store=False`` (nothing is stored per step; ``u_nn`` and ``flag`` are ``None`` without recovery);
    * ``x_final (M,B,5)``: the unperturbed state after step T;
    * ``traj_stats (M,B,6)`` fp64: per trajectory, with e = ``x[:,t+1,1] - ref[:,t]`` (the record as stored, measurement
      noise included), sum |e|, sum e^2, max |e|, sum |u|, sum_{t>=1} (u_t - u_{t-1})^2, and the worst violation
      max_t max(p1_lo - p1, p1 - p1_hi, p2_lo - p2, p2 - p2_hi) of the records' pressures (Pa);
    * ``traj_counts (M,B,3)`` int32: steps with violation > 0, steps flagged 1, steps flagged 2;
    * ``metrics``: ``(M,)`` fp64 tensors keyed ``MAE``, ``RMSE``, ``R2``, ``Command`` (the reference's ``results_dict``
      keys; speed tracking over all B*T steps, mean |u|), ``max_err``, ``du_rms``, ``viol_max``, ``viol_frac``,
      ``flag1_frac``, ``flag2_frac``."""

    def __init__(self, bank, scalers: dict, ts: float = TS_REFERENCE, substeps: int = SUBSTEPS_REFERENCE,
                 smooth: bool = True):
        for name in ("w_inp", "b_inp", "w_out"):
            if not hasattr(bank, name):
                raise TypeError(f"ClosedLoopBank needs a ControllerBank (stacked w_inp, b_inp, w_out); got {type(bank).__name__}")
        super().__init__(scalers, ts, substeps, smooth)
        self.bank = bank

    @classmethod
    def of_loop(cls, loop: "ClosedLoop") -> "ClosedLoopBank":
        """The bank of ONE model that runs ``loop``'s controller with its scales and step."""
        w_inp, b_inp, w_out = (p.detach() for p in _controller_params(loop.controller))
        bank = types.SimpleNamespace(w_inp=w_inp[None], b_inp=b_inp[None], w_out=w_out.reshape(1, -1))
        return cls(bank, loop, loop.ts, loop.substeps, loop.smooth)

    def run(self, x0: torch.Tensor, ref: torch.Tensor, process_noise: torch.Tensor | None = None,
            meas_noise: torch.Tensor | None = None, feasibility: FeasibilityRecovery | None = None, store: bool = True,
            p_bounds=None, plant_params=None, differentiable: bool = False):
        """``x0 (B,5)`` or ``(M,B,5)``, ``ref (B,T)`` or ``(M,B,T)``, each noise ``(B,T,5)`` or ``(M,B,T,5)``: without
        the leading M one copy is shared by all models (and read once from memory, not expanded). ``p_bounds``:
        ``((p1_lo, p1_hi), (p2_lo, p2_hi))`` in Pa for the violation statistics; default the ``feasibility``'s own
        bounds, otherwise 0 and 32e6. ``store=False`` skips every per-step store; the statistics, ``x_final`` and
        ``metrics`` are the storing run's bit for bit.

        ``plant_params``: the press each trajectory's loop steps (the TRUE plant) — a :class:`~.plant.PressParams` or a
        ``(28,)`` row for all, a ``(B,28)`` table shared by the models, or ``(M,B,28)``; shared layouts are read as they
        lie, through zero strides, not expanded. The projection of ``feasibility`` integrates that object's
        ``model_params`` (default: the reference's press), one set for the launch — plant and model need not agree, which
        is what the violation statistics then measure. ``None`` (and no ``model_params``) is the call as it always was:
        ``fcr_closed_loop_run_bank`` and its kernels; otherwise ``fcr_closed_loop_run_bank_press``.

        ``differentiable=True``: ``x`` and ``u`` of the returned dict are attached to the bank's
        stacked ``w_inp``, ``b_inp``, ``w_out`` and to ``x0`` (a shared ``(B,5)`` ``x0`` receives the sum over the
        models); under ``torch.no_grad()`` they come back detached. The forward is the launch above, same bits; the
        backward is the bank's adjoint in one launch (``fcr_closed_loop_bank_vjp``, :func:`bank_vjp`) with
        :meth:`ClosedLoop.run`'s conventions. ``plant_params`` is taken in every form, as constants. Raises
        ``ValueError`` with noise, ``feasibility`` or ``store=False``. Every other entry of the dict is detached."""
        if differentiable:
            given = {"process_noise": process_noise, "meas_noise": meas_noise, "feasibility": feasibility,
                     "store=False": None if store else False}
            for name, v in given.items():
                if v is not None:
                    raise ValueError(f"ClosedLoopBank.run(differentiable=True) does not take {name}: the adjoint covers "
                                     "the stored noise-free loop without recovery (DESIGN.md §7.13, §7.16); under noise: "
                                     "run_differentiable (§7.18)")
            if torch.is_grad_enabled():
                holder = {}
                x, u = _ClosedLoopBankGrad.apply(self, holder, p_bounds, x0, ref, plant_params, self.bank.w_inp,
                                                 self.bank.b_inp, self.bank.w_out)
                return {**holder["out"], "x": x, "u": u}
        return self._launch(x0, ref, process_noise, meas_noise, feasibility, store, p_bounds, plant_params)

    def run_differentiable(self, x0: torch.Tensor, ref: torch.Tensor, process_noise: torch.Tensor | None = None,
                           meas_noise: torch.Tensor | None = None, plant_params=None, truncate: int = 0, p_bounds=None,
                           _weights=None):
        """:meth:`run` under pre-drawn noise, attached to the graph: :meth:`run`'s dict with ``x`` and
        ``u`` attached to the bank's stacked parameters and to ``x0``, plus ``x_state (M,B,T+1,5)``, the unperturbed
        states (detached; without ``meas_noise`` it is the record). ``process_noise`` / ``meas_noise``: ``(B,T,5)``
        shared or ``(M,B,T,5)``, constants — no gradient reaches them (:func:`harness_noise`, :func:`device_noise`).
        ``x``, ``u`` and the metrics are ``run(process_noise=, meas_noise=)``'s bit for bit; without noise the call is
        ``run(differentiable=True)``. Under ``torch.no_grad()`` everything comes back detached.

        The backward is one reverse launch (``fcr_closed_loop_bank_vjp_noise``): the incoming gradients are those on the
        RECORD ``x`` (``= x_state + v``, so they are the state's too); the controller's chain and masks are taken from the
        record it read; the plant is linearised at the state, with the step's noise at every RK4 stage. ``truncate = K``:
        truncated back-propagation, as :func:`bank_vjp`'s. Conventions at the singular points: :meth:`ClosedLoop.run`'s.
        Not covered: feasibility recovery, gradients with respect to the noise, ``ref`` or the press."""
        if int(truncate) != truncate or int(truncate) < 0:
            raise ValueError(f"run_differentiable: truncate = {truncate!r} must be an integer >= 0 (0 = none)")
        weights = (self.bank.w_inp, self.bank.b_inp, self.bank.w_out) if _weights is None else _weights
        if not torch.is_grad_enabled():
            return self._launch(x0, ref, process_noise, meas_noise, None, True, p_bounds, plant_params,
                                with_state=True)
        holder = {}
        x, u = _NoisyBankGrad.apply(self, holder, p_bounds, int(truncate), x0, ref, process_noise, meas_noise, plant_params,
                                    *weights)
        return {**holder["out"], "x": x, "u": u}

    def _launch(self, x0, ref, process_noise, meas_noise, feasibility, store, p_bounds, plant_params, with_state=False):
        """The forward launch of :meth:`run`. ``with_state``: the returned dict gains ``x_state`` — under ``meas_noise``
        stored by the launch itself (``fcr_closed_loop_run_bank_press_state``), otherwise the record."""
        M = self.bank.w_inp.shape[0]
        dev, B, T, stacked, out, prefix, keep = self._prepare(M, (self.bank.w_inp, self.bank.b_inp, self.bank.w_out), x0, ref,
                                                              process_noise, meas_noise, feasibility, store)
        if plant_params is not None and _press_shape(plant_params) not in ((28,), (B, 28), (M, B, 28)):
            raise ValueError(f"plant_params must be a PressParams, (28,), (B,28) = {(B, 28)} or (M,B,28) = {(M, B, 28)}, "
                             f"got shape {_press_shape(plant_params)}")
        if p_bounds is None:
            p_bounds = (feasibility.p1, feasibility.p2) if feasibility is not None else ((0.0, 32e6), (0.0, 32e6))
        (p1_lo, p1_hi), (p2_lo, p2_hi) = p_bounds
        new = lambda *shape, dtype=torch.float64: torch.empty(M, B, *shape, dtype=dtype, device=dev)
        out["x_final"], out["traj_stats"], out["traj_counts"] = new(5), new(6), new(3, dtype=torch.int32)
        summary = torch.empty(M, 10, dtype=torch.float64, device=dev)
        p = lambda t: t.data_ptr()
        stride = lambda name, per: per if stacked[name] else 0
        args = _native.FcrClosedLoopBank(
            *prefix, M, stride("x0", B * 5), stride("ref", B * T), stride("process_noise", B * T * 5),
            stride("meas_noise", B * T * 5), float(p1_lo), float(p1_hi), float(p2_lo), float(p2_hi), p(out["traj_stats"]),
            p(out["traj_counts"]), p(out["x_final"]), p(summary))
        model = None if feasibility is None else feasibility.model_params
        name, extra = "fcr_closed_loop_run_bank", ()
        if with_state and meas_noise is not None:
            table = None if plant_params is None else as_press_table(plant_params, dev, "plant_params")
            out["x_state"] = torch.empty(M, B, T + 1, 5, dtype=torch.float64, device=dev)
            name = "fcr_closed_loop_run_bank_press_state"
            extra = (None if table is None else p(table), B * 28 if table is not None and table.dim() == 3 else 0,
                     28 if table is not None and table.dim() >= 2 else 0, None, p(out["x_state"]))
        elif plant_params is not None or model is not None:
            table = as_press_table(PressParams() if plant_params is None else plant_params, dev, "plant_params")
            m_struct = None if model is None else model.struct()
            name = "fcr_closed_loop_run_bank_press"
            extra = (p(table), B * 28 if table.dim() == 3 else 0, 28 if table.dim() >= 2 else 0,
                     None if m_struct is None else ctypes.byref(m_struct))
        _native.check(getattr(_native.load(), name)(ctypes.byref(args), *extra, _native.stream(dev)), name)
        if M == 0 or B == 0:
            summary.zero_()
        out["metrics"] = {k: summary[:, i] for i, k in enumerate(METRIC_KEYS)}
        if with_state and "x_state" not in out:
            out["x_state"] = out["x"]
        return out

    def loop(self, x0: torch.Tensor, ref: torch.Tensor, simulator, model_scalers: dict,
             process_noise: torch.Tensor | None = None, meas_noise: torch.Tensor | None = None,
             lstm_noise: torch.Tensor | None = None, feasibility: FeasibilityRecovery | None = None, store: bool = True,
             p_bounds=None, plant_params=None):
        """:meth:`ClosedLoop.loop` for every model: ``(results, results_LSTM)`` keyed as there, every tensor with a
        leading model dimension (``ref`` expanded to ``(M,B,T)``), plus ``results['metrics']``. The surrogate is shared
        by the models, so its track is ONE ``simulate_rollout`` launch on the ``(M*B)`` stack of rows. ``lstm_noise``:
        ``(B,T,4)`` shared or ``(M,B,T,4)``. The tracks are built from the stored trajectories: ``store`` must be True.
        ``plant_params`` (:meth:`run`) is the press's own; the surrogate's track is unaffected by it."""
        if not store:
            raise ValueError("ClosedLoopBank.loop builds both tracks from the stored trajectories: store=True is required")
        s_in, s_out = _model_scales(model_scalers)
        r = self.run(x0, ref, process_noise, meas_noise, feasibility, store=True, p_bounds=p_bounds, plant_params=plant_params)
        x, u = r["x"], r["u"]
        M, B, T = u.shape
        results = {"y": x[..., 0], "y_dot": x[..., 1], "p1": x[..., 2], "p2": x[..., 3], "z": x[..., 4],
                   "ref": ref.to(torch.float64).expand(M, B, T), "u": u, "metrics": r["metrics"]}
        if feasibility is not None:
            results["u_nn"], results["feas_flag"] = r["u_nn"], r["flag"]
        if lstm_noise is not None:
            if _per_model("lstm_noise", lstm_noise, M, (B, T, 4)):
                lstm_noise = lstm_noise.reshape(M * B, T, 4)
            else:
                lstm_noise = lstm_noise.expand(M, B, T, 4).reshape(M * B, T, 4)
        track = _shadow_track(x[:, :, 0, 1:5].reshape(M * B, 4), u.reshape(M * B, T), simulator, s_in, s_out, lstm_noise)
        track = track.reshape(M, B, T + 1, 4)
        results_lstm = {"y_dot": track[..., 0], "p1": track[..., 1], "p2": track[..., 2], "z": track[..., 3]}
        return results, results_lstm


class _ClosedLoopBankGrad(torch.autograd.Function):
    """:meth:`ClosedLoopBank.run` attached to the graph: the forward is the plain launch, the backward
    ``fcr_closed_loop_bank_vjp`` on the stored run. ``holder['out']`` receives the run's whole dict."""

    @staticmethod
    def forward(ctx, loop, holder, p_bounds, x0, ref, plant_params, w_inp, b_inp, w_out):
        if torch.is_tensor(plant_params):
            plant_params = plant_params.detach()
        out = loop.run(x0, ref, p_bounds=p_bounds, plant_params=plant_params)
        holder["out"] = dict(out)
        x, u = out["x"], out["u"]
        dev = x.device
        ctx.loop = loop
        ctx.tab = None if plant_params is None else as_press_table(plant_params, dev, "plant_params")
        ctx.like = tuple((t.shape, t.device, t.dtype) for t in (x0, w_inp, b_inp, w_out))
        ctx.save_for_backward(x, u, ref.to(torch.float64).contiguous(),
                              *(p.detach().to(device=dev, dtype=torch.float32).contiguous() for p in (w_inp, b_inp, w_out)))
        return x, u

    @staticmethod
    def backward(ctx, g_x, g_u):
        x, u, ref, w_inp, b_inp, w_out = ctx.saved_tensors
        g = bank_vjp(ctx.loop, x, u, ref, g_x, g_u, (w_inp, b_inp, w_out), ctx.tab, want_x0=ctx.needs_input_grad[3])
        like = lambda t, to: t.reshape(to[0]).to(device=to[1], dtype=to[2])
        x0_, wi_, bi_, wo_ = ctx.like
        g_x0 = None
        if ctx.needs_input_grad[3]:
            g_x0 = like(g["g_x0"] if len(x0_[0]) == 3 else g["g_x0"].sum(0), x0_)   # a shared x0: the sum over the models
        return (None, None, None, g_x0, None, None, like(g["g_w_inp"], wi_), like(g["g_b_inp"], bi_), like(g["g_w_out"], wo_))


class _NoisyBankGrad(torch.autograd.Function):
    """:meth:`ClosedLoopBank.run_differentiable` attached to the graph: the forward is the bank's launch under the given
    noise (storing the states beside the record under measurement noise), the backward :func:`bank_vjp` on the stored run
    with that noise. ``holder['out']`` receives the run's whole dict, ``x_state`` included."""

    @staticmethod
    def forward(ctx, loop, holder, p_bounds, truncate, x0, ref, process_noise, meas_noise, plant_params, w_inp, b_inp, w_out):
        if torch.is_tensor(plant_params):
            plant_params = plant_params.detach()
        out = loop._launch(x0, ref, process_noise, meas_noise, None, True, p_bounds, plant_params, with_state=True)
        holder["out"] = dict(out)
        x, u = out["x"], out["u"]
        dev = x.device
        ctx.loop, ctx.truncate = loop, truncate
        ctx.tab = None if plant_params is None else as_press_table(plant_params, dev, "plant_params")
        ctx.like = tuple((t.shape, t.device, t.dtype) for t in (x0, w_inp, b_inp, w_out))
        ctx.noisy = (process_noise is not None, meas_noise is not None)
        ctx.save_for_backward(x, u, ref.to(torch.float64).contiguous(),
                              *(p.detach().to(device=dev, dtype=torch.float32).contiguous() for p in (w_inp, b_inp, w_out)),
                              process_noise.detach() if ctx.noisy[0] else None, out["x_state"] if ctx.noisy[1] else None)
        return x, u

    @staticmethod
    def backward(ctx, g_x, g_u):
        x, u, ref, w_inp, b_inp, w_out, process_noise, x_state = ctx.saved_tensors
        g = bank_vjp(ctx.loop, x, u, ref, g_x, g_u, (w_inp, b_inp, w_out), ctx.tab, truncate=ctx.truncate,
                     want_x0=ctx.needs_input_grad[4], process_noise=process_noise, x_state=x_state)
        like = lambda t, to: t.reshape(to[0]).to(device=to[1], dtype=to[2])
        x0_, wi_, bi_, wo_ = ctx.like
        g_x0 = None
        if ctx.needs_input_grad[4]:
            g_x0 = like(g["g_x0"] if len(x0_[0]) == 3 else g["g_x0"].sum(0), x0_)   # a shared x0: the sum over the models
        return (None, None, None, None, g_x0, None, None, None, None, like(g["g_w_inp"], wi_), like(g["g_b_inp"], bi_),
                like(g["g_w_out"], wo_))


def device_noise(B: int, T: int, process_std, meas_std, device, generator: torch.Generator | None = None, M: int | None = None):
    """Noise for training, drawn with torch on ``device``: ``(w, v)``, each fp64 ``(B,T,5)`` (``M`` given: ``(M,B,T,5)``, a
    draw per model) or ``None`` where its standard deviations (a number or five, per state) are all zero or ``None``.
    ``w = process_std * N(0,1)`` in the units of x_dot, ``v = meas_std * N(0,1)`` in the units of the state, as
    :meth:`ClosedLoopBank.run` takes them. It does NOT follow the reference's draw order (one numpy stream, 14 values per
    step, trajectory by trajectory): two runs from equal ``generator`` states agree with each other and with nothing else.
    :func:`harness_noise` is the one that reproduces the harness's draws."""
    shape = ((int(B), int(T), 5) if M is None else (int(M), int(B), int(T), 5))

    def draw(std, name):
        if std is None:
            return None
        s = torch.as_tensor(std, dtype=torch.float64).reshape(-1)
        if s.numel() not in (1, 5) or bool((s < 0).any()) or not bool(torch.isfinite(s).all()):
            raise ValueError(f"device_noise: {name} must be one or five finite standard deviations >= 0, got {std!r}")
        if not bool((s > 0).any()):
            return None
        return torch.randn(shape, dtype=torch.float64, device=device, generator=generator) * s.to(device)

    return draw(process_std, "process_std"), draw(meas_std, "meas_std")


def _bank_adjoint(who, loop, x, u, ref, weights, plant_params, truncate, want_x0, want_grads=True):
    """What :func:`bank_vjp` and :func:`bank_loss_vjp` share: the checks, the conversions, the outputs, the workspace and
    the ``fcr_closed_loop_bank_grad`` of the call. Returns ``(args, out, ws, keep)``."""
    dev = x.device
    if dev.type != "cuda":
        raise RuntimeError(f"ClosedLoopBank runs on a ROCm device only (x on {x.device})")
    if u.dim() != 3 or tuple(x.shape) != (*u.shape[:2], u.shape[2] + 1, 5):
        raise ValueError(f"{who}: x must be (M,B,T+1,5) and u (M,B,T); got {tuple(x.shape)}, {tuple(u.shape)}")
    M, B, T = u.shape
    if tuple(ref.shape) not in ((B, T), (M, B, T)):
        raise ValueError(f"{who}: ref must be (B,T) = {(B, T)} or (M,B,T) = {(M, B, T)}, got {tuple(ref.shape)}")
    if int(truncate) < 0:
        raise ValueError(f"{who}: truncate = {truncate} must be >= 0 (0 = none)")
    f64 = lambda t: t.to(device=dev, dtype=torch.float64).contiguous()
    x, u, ref = f64(x), f64(u), f64(ref)
    if weights is None:
        weights = (loop.bank.w_inp, loop.bank.b_inp, loop.bank.w_out)
    w_inp, b_inp, w_out = (t.detach().to(device=dev, dtype=torch.float32).contiguous() for t in weights)
    H = w_inp.shape[-2]
    if tuple(w_inp.shape) != (M, H, 3) or tuple(b_inp.shape) != (M, H) or tuple(w_out.shape) != (M, H):
        raise ValueError(f"{who}: the bank's parameters must be (M,H,3), (M,H), (M,H) with M = {M}; got "
                         f"{tuple(w_inp.shape)}, {tuple(b_inp.shape)}, {tuple(w_out.shape)}")
    tab = None if plant_params is None else as_press_table(plant_params, dev, "plant_params")
    if tab is not None and tuple(tab.shape) not in ((28,), (B, 28), (M, B, 28)):
        raise ValueError(f"plant_params must be a PressParams, (28,), (B,28) = {(B, 28)} or (M,B,28) = {(M, B, 28)}, "
                         f"got shape {tuple(tab.shape)}")
    new = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)
    out = {}
    if want_grads:
        out = {"g_x0": new(M, B, 5) if want_x0 else None, "dv": new(M, B, T), "g_w_inp": new(M, H, 3),
               "g_b_inp": new(M, H), "g_w_out": new(M, H)}
    lib = _native.load()
    size = ctypes.c_size_t(0)
    _native.check(lib.fcr_closed_loop_bank_vjp_workspace_size(M, B, T, H, ctypes.byref(size)),
                  "fcr_closed_loop_bank_vjp_workspace_size")
    ws = torch.empty(max(size.value, 8), dtype=torch.uint8, device=dev)
    p = lambda t: None if t is None else t.data_ptr()
    args = _native.FcrClosedLoopBankGrad(
        M, B, T, loop.ts, loop.substeps, int(loop.smooth), p(ref), B * T if ref.dim() == 3 else 0, p(w_inp), p(b_inp),
        p(w_out), H, (ctypes.c_double * 2)(*loop.in_scale), loop.ref_scale, loop.out_scale, p(x), p(u), p(tab),
        B * 28 if tab is not None and tab.dim() == 3 else 0, 28 if tab is not None and tab.dim() >= 2 else 0,
        int(truncate), p(out.get("g_x0")), p(out.get("dv")), p(out.get("g_w_inp")), p(out.get("g_b_inp")),
        p(out.get("g_w_out")))
    return args, out, ws, (x, u, ref, w_inp, b_inp, w_out, tab)


def _bank_noise(who, process_noise, x_state, x, keep):
    """The ``fcr_bank_noise`` of a noisy run's adjoint, or ``None`` when the run had no noise:
    ``process_noise`` ``(B,T,5)`` shared or ``(M,B,T,5)``, ``x_state`` the forward's states, shaped as ``x``."""
    if process_noise is None and x_state is None:
        return None
    dev, (M, B, T) = x.device, x.shape[:2] + (x.shape[2] - 1,)
    f64 = lambda t: t.detach().to(device=dev, dtype=torch.float64).contiguous()
    stride = 0
    if process_noise is not None:
        stride = B * T * 5 if _per_model("process_noise", process_noise, M, (B, T, 5)) else 0
        process_noise = f64(process_noise)
    if x_state is not None:
        if tuple(x_state.shape) != tuple(x.shape):
            raise ValueError(f"{who}: x_state must have x's shape {tuple(x.shape)}, got {tuple(x_state.shape)}")
        x_state = f64(x_state)
    keep.extend((process_noise, x_state))
    p = lambda t: None if t is None else t.data_ptr()
    return _native.FcrBankNoise(p(process_noise), stride, p(x_state))


def bank_vjp(loop: "ClosedLoopBank", x, u, ref, g_x, g_u, weights=None, plant_params=None, truncate: int = 0,
             want_x0: bool = True, process_noise=None, x_state=None) -> dict:
    """:func:`loop_vjp` for the M models of a :class:`ClosedLoopBank` in one reverse launch (``fcr_closed_loop_bank_vjp``):
    from the stored ``x (M,B,T+1,5)``, ``u (M,B,T)``, the run's ``ref`` (``(B,T)`` shared or ``(M,B,T)``) and the incoming
    ``g_x``, ``g_u`` of those shapes, a dict of fp64 tensors ``g_x0 (M,B,5)`` (``None`` with ``want_x0=False``),
    ``dv (M,B,T)``, ``g_w_inp (M,H,3)``, ``g_b_inp (M,H)``, ``g_w_out (M,H)`` — model m's are :func:`loop_vjp`'s for that
    model alone. ``weights``: the bank's three stacked parameters as the run read them (default: the bank's now);
    ``plant_params``: the run's, in any of its four forms. ``truncate = K > 0``: the states at ``t = K, 2K, ... < T``
    count as constants for the step that starts from them (``x = x.detach()`` there).

    ``process_noise`` / ``x_state``: the run was made under noise (:meth:`ClosedLoopBank.run_differentiable`; DESIGN.md
    §7.18) — its process noise, ``(B,T,5)`` shared or ``(M,B,T,5)``, and the unperturbed states that run returned
    (``None``: no measurement noise, the record is the state). ``g_x`` is then the gradient on the record; the plant is
    linearised at the state with the step's noise (``fcr_closed_loop_bank_vjp_noise``)."""
    args, out, ws, keep = _bank_adjoint("bank_vjp", loop, x, u, ref, weights, plant_params, truncate, want_x0)
    dev, (M, B, T) = keep[0].device, keep[1].shape
    if tuple(g_x.shape) != (M, B, T + 1, 5) or tuple(g_u.shape) != (M, B, T):
        raise ValueError(f"bank_vjp: g_x must be (M,B,T+1,5) and g_u (M,B,T); got {tuple(g_x.shape)}, {tuple(g_u.shape)}")
    gx, gu = (t.to(device=dev, dtype=torch.float64).contiguous() for t in (g_x, g_u))
    held = []
    noise = _bank_noise("bank_vjp", process_noise, x_state, keep[0], held)
    if noise is not None:
        _native.check(_native.load().fcr_closed_loop_bank_vjp_noise(
            ctypes.byref(args), ctypes.byref(noise), ctypes.c_void_p(gx.data_ptr()), ctypes.c_void_p(gu.data_ptr()),
            ctypes.c_void_p(ws.data_ptr()), ws.numel(), _native.stream(dev)), "fcr_closed_loop_bank_vjp_noise")
        return out
    _native.check(_native.load().fcr_closed_loop_bank_vjp(
        ctypes.byref(args), ctypes.c_void_p(gx.data_ptr()), ctypes.c_void_p(gu.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
        ws.numel(), _native.stream(dev)), "fcr_closed_loop_bank_vjp")
    return out


def bank_loss_vjp(loop: "ClosedLoopBank", x, u, ref, terms_rows, p_scale, u_prev=None, weights=None, plant_params=None,
                  truncate: int = 0, want_x0: bool = True, value_only: bool = False, process_noise=None,
                  x_state=None) -> dict:
    """The MPC loss on the stored run of a bank and its gradient in one reverse launch
    (``fcr_closed_loop_bank_loss_vjp``; the loss: :class:`~.press_loss.PressLoss`). ``terms_rows``: one row
    ``(alpha, p1_lo, p1_hi, p2_lo, p2_hi, weight)`` for all models or one per model; ``p_scale``: the two pressure
    scales; ``u_prev``: ``(B,)`` shared or ``(M,B)``, or ``None``. Returns :func:`bank_vjp`'s dict and ``cost (M,B)``,
    ``loss (M,)``; ``value_only=True``: those two alone, nothing is differentiated. ``process_noise`` / ``x_state``: the
    run was made under noise, as for :func:`bank_vjp` (``fcr_closed_loop_bank_loss_vjp_noise``); the loss is the record's."""
    args, out, ws, keep = _bank_adjoint("bank_loss_vjp", loop, x, u, ref, weights, plant_params, truncate, want_x0,
                                        want_grads=not value_only)
    dev, (M, B, T) = keep[0].device, keep[1].shape
    rows = np.ascontiguousarray(np.asarray(terms_rows, dtype=np.float64).reshape(-1, 6))
    if rows.shape[0] not in (1, M):
        raise ValueError(f"bank_loss_vjp: {rows.shape[0]} terms rows for a bank of {M} models")
    table = torch.tensor(rows, dtype=torch.float64, device=dev)
    if u_prev is not None:
        if tuple(u_prev.shape) not in ((B,), (M, B)):
            raise ValueError(f"bank_loss_vjp: u_prev must be (B,) = {(B,)} or (M,B) = {(M, B)}, got {tuple(u_prev.shape)}")
        u_prev = u_prev.detach().to(device=dev, dtype=torch.float64).contiguous()
    out["cost"] = torch.zeros(M, B, dtype=torch.float64, device=dev)
    out["loss"] = torch.zeros(M, dtype=torch.float64, device=dev)
    loss = _native.FcrPressLoss(
        table.data_ptr(), 6 if rows.shape[0] > 1 else 0, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
        (ctypes.c_double * 2)(float(p_scale[0]), float(p_scale[1])), None if u_prev is None else u_prev.data_ptr(),
        B if u_prev is not None and u_prev.dim() == 2 else 0, int(bool(value_only)), out["cost"].data_ptr(),
        out["loss"].data_ptr())
    held = []
    noise = _bank_noise("bank_loss_vjp", process_noise, x_state, keep[0], held)
    if noise is not None:
        _native.check(_native.load().fcr_closed_loop_bank_loss_vjp_noise(
            ctypes.byref(args), ctypes.byref(noise), ctypes.byref(loss), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
            _native.stream(dev)), "fcr_closed_loop_bank_loss_vjp_noise")
        return out
    _native.check(_native.load().fcr_closed_loop_bank_loss_vjp(
        ctypes.byref(args), ctypes.byref(loss), ctypes.c_void_p(ws.data_ptr()), ws.numel(), _native.stream(dev)),
        "fcr_closed_loop_bank_loss_vjp")
    return out
