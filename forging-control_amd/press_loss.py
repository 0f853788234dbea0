"""Training controllers on the press itself: the MPC loss on the closed-loop record, fused with the
adjoint of the loop for a whole bank, and the training loop on top of it.

:class:`PressLoss` evaluates, in fp64 and for every model m of a bank on its ``B`` trajectories of ``T`` steps,

* ``e_t = (x[t+1,1] - ref[t]) / s_v``, ``d_t = (u_t - u_{t-1}) / s_u`` (``d_0 = (u_0 - u_prev) / s_u``, or 0 without
  ``u_prev``), ``c_t = w (relu(lo1 - P1) + relu(P1 - hi1) + relu(lo2 - P2) + relu(P2 - hi2))`` with
  ``P1 = x[t+1,2] / s_p1``, ``P2 = x[t+1,3] / s_p2``;
* ``cost[m,b] = (1/T) sum_t (e_t^2 + alpha d_t^2 + c_t)`` and ``loss[m] = (1/B) sum_b cost[m,b]``

with ``s_v``, ``s_u`` the loop's own ``ref_scale`` and ``out_scale``, ``(s_p1, s_p2) = p_scale`` (the surrogate output
scaler's ``max_abs_[1:3]``, so that :meth:`LossTerms.from_scalers` gives the bounds of the surrogate's loss) and
``(alpha, lo1, hi1, lo2, hi2, w)`` each model's :meth:`LossTerms.as_row`. A training step is two launches and the
parameter kernels: the loop's forward launch as it always was, then ONE reverse launch that forms the loss's cotangents
in registers from the record it reads anyway (``fcr_closed_loop_bank_loss_vjp``, csrc/fcr_press_train.h).
:func:`train_on_press` is :func:`~.many.train_models` on the press; with a ``(B,28)`` or ``(M,B,28)`` table per batch
it is domain randomisation.
"""
from __future__ import annotations

import torch

from .closed_loop import ClosedLoop, ClosedLoopBank, bank_loss_vjp
from .functions import _controller_params
from .loss_terms import LossTerms, resolve


class PressLoss:
    """``PressLoss(loop, p_scale, terms=None, alpha=0.1, truncate=0)``: ``loop`` a :class:`ClosedLoopBank`, or a
    :class:`ClosedLoop` (a bank of one). ``terms``: one :class:`LossTerms` for all models or one per model (``None``: the
    defaults); ``alpha`` fills in where a LossTerms has none. ``truncate = K > 0`` is truncated back-propagation: the
    states at ``t = K, 2K, ... < T`` count as constants for the step that starts from them (``x = x.detach()`` there);
    the loss's value does not depend on it.

    ``forward(x0, ref, plant_params=None, u_prev=None)`` -> ``(loss (M,), features)``, ``features`` holding
    ``cost (M,B)``, the detached ``x (M,B,T+1,5)`` and ``u (M,B,T)`` and the run's ``metrics``
    (:meth:`ClosedLoopBank.run`). ``loss`` is attached to the bank's stacked parameters (a single loop: its controller's)
    and to ``x0`` (a shared ``(B,5)`` receives the sum over the models); ``plant_params`` in every form and ``u_prev``
    (``(B,)`` or ``(M,B)``) are constants. The gradients are computed in the forward (each model's loss is a scalar, so
    the backward only multiplies model m's by ``g_loss[m]``): ``loss.sum().backward()`` trains every model on its own
    loss. Under ``torch.no_grad()`` only the forward launch and the loss's value kernel run.

    ``forward(..., process_noise=None, meas_noise=None)``: the loop runs under that pre-drawn noise, ``(B,T,5)`` shared
    by the models or ``(M,B,T,5)`` (:func:`~.closed_loop.harness_noise`, :func:`~.closed_loop.device_noise`):
    still one forward launch and one fused reverse launch. The loss is evaluated on the record ``x`` (measurement noise
    included), as the run's metrics are; the noise is a constant. ``features`` then also holds ``x_state``."""

    def __init__(self, loop, p_scale, terms=None, alpha: float = 0.1, truncate: int = 0):
        if not isinstance(loop, (ClosedLoop, ClosedLoopBank)):
            raise TypeError(f"PressLoss needs a ClosedLoop or a ClosedLoopBank, got {type(loop).__name__}")
        try:
            s1, s2 = (float(v) for v in p_scale)
        except (TypeError, ValueError):
            raise ValueError(f"PressLoss: p_scale must be a pair of positive numbers, got {p_scale!r}") from None
        if not (0.0 < s1 < float("inf") and 0.0 < s2 < float("inf")):
            raise ValueError(f"PressLoss: p_scale = ({s1}, {s2}) must be positive and finite")
        if int(truncate) != truncate or int(truncate) < 0:
            raise ValueError(f"PressLoss: truncate = {truncate!r} must be an integer >= 0 (0 = none)")
        self.loop, self.p_scale, self.alpha, self.truncate = loop, (s1, s2), float(alpha), int(truncate)
        terms = LossTerms() if terms is None else terms
        self.terms = resolve(terms, None if isinstance(terms, LossTerms) else self.n_models)

    @property
    def n_models(self) -> int:
        return 1 if isinstance(self.loop, ClosedLoop) else self.loop.bank.w_inp.shape[0]

    def rows(self):
        """The models' rows ``(alpha, p1_lo, p1_hi, p2_lo, p2_hi, weight)``: one for all, or one per model."""
        terms = (self.terms,) if isinstance(self.terms, LossTerms) else self.terms
        return [t.as_row(self.alpha) for t in terms]

    def _bank(self):
        """``(bank loop, its three stacked parameters attached to the graph)``."""
        if isinstance(self.loop, ClosedLoopBank):
            b = self.loop.bank
            return self.loop, (b.w_inp, b.b_inp, b.w_out)
        w_inp, b_inp, w_out = _controller_params(self.loop.controller)
        return ClosedLoopBank.of_loop(self.loop), (w_inp[None], b_inp[None], w_out.reshape(1, -1))

    def forward(self, x0, ref, plant_params=None, u_prev=None, process_noise=None, meas_noise=None):
        if plant_params is None and isinstance(self.loop, ClosedLoop):
            plant_params = self.loop.plant_params
        if isinstance(self.loop, ClosedLoop) and (x0.dim() != 2 or ref.dim() != 2):
            raise ValueError(f"x0 must be (B,5) and ref (B,T); got {tuple(x0.shape)}, {tuple(ref.shape)}")
        bank_loop, weights = self._bank()
        features = {}
        loss = _PressLossFn.apply(self, bank_loop, features, x0, ref, plant_params, u_prev, *weights, process_noise,
                                  meas_noise)
        return loss, features

    __call__ = forward


class _PressLossFn(torch.autograd.Function):
    """Forward: the bank's launch, then the fused reverse launch, whose gradients are stashed (grad mode off: the value
    kernel alone). Backward: model m's gradients times ``g_loss[m]``."""

    @staticmethod
    def forward(ctx, pl, bank_loop, features, x0, ref, plant_params, u_prev, w_inp, b_inp, w_out, process_noise=None,
                meas_noise=None):
        if torch.is_tensor(plant_params):
            plant_params = plant_params.detach()
        noisy = process_noise is not None or meas_noise is not None
        if noisy:   # the same launch under noise; under measurement noise it stores the states beside the record
            r = bank_loop._launch(x0.detach(), ref, process_noise, meas_noise, None, True, None, plant_params, with_state=True)
        else:
            r = bank_loop.run(x0.detach(), ref, plant_params=plant_params)
        needs = ctx.needs_input_grad
        grads = any(needs[i] for i in (3, 7, 8, 9))
        g = bank_loss_vjp(bank_loop, r["x"], r["u"], ref, pl.rows(), pl.p_scale, u_prev,
                          tuple(t.detach() for t in (w_inp, b_inp, w_out)), plant_params, pl.truncate, want_x0=needs[3],
                          value_only=not grads, process_noise=process_noise,
                          x_state=r["x_state"] if meas_noise is not None else None)
        features.update(cost=g["cost"], x=r["x"], u=r["u"], metrics=r["metrics"])
        if noisy:
            features["x_state"] = r["x_state"]
        ctx.grads = grads
        if grads:
            ctx.like = tuple((t.shape, t.device, t.dtype) for t in (x0, w_inp, b_inp, w_out))
            ctx.stash = (g["g_x0"], g["g_w_inp"], g["g_b_inp"], g["g_w_out"])   # g_x0 (M,B,5), or None: not wanted
        return g["loss"]

    @staticmethod
    def backward(ctx, g_loss):
        if not ctx.grads:
            return (None,) * 12
        g_x0, g_wi, g_bi, g_wo = ctx.stash
        gl = g_loss.to(torch.float64)
        like = lambda t, to: t.reshape(to[0]).to(device=to[1], dtype=to[2])
        x0_, wi_, bi_, wo_ = ctx.like
        out_x0 = None
        if g_x0 is not None:
            g_x0 = g_x0 * gl[:, None, None]
            out_x0 = like(g_x0 if len(x0_[0]) == 3 else g_x0.sum(0), x0_)   # a shared x0: the sum over the models
        return (None, None, None, out_x0, None, None, None, like(g_wi * gl[:, None, None], wi_),
                like(g_bi * gl[:, None], bi_), like(g_wo * gl[:, None], wo_), None, None)


def train_on_press(batches, bank_loop, press_loss: PressLoss, optimizer, plant_sampler=None, step=None, noise_sampler=None):
    """:func:`~.many.train_models` on the press: for every batch ``(x0, ref)`` or ``(x0, ref, u_prev)`` one training
    step of all the bank's models — the forward launch, the fused reverse launch, ``losses.sum().backward()`` (the
    models are independent: each receives the gradient of its own loss) and ``optimizer.step()``.

    ``bank_loop``: the :class:`ClosedLoopBank` (or :class:`ClosedLoop`) that ``press_loss`` was built on.
    ``plant_sampler(B)``: called once per batch, returns that batch's press — a ``(B,28)`` or ``(M,B,28)`` table (domain
    randomisation, for example ``PressParams.sample``), or anything else ``plant_params`` takes; ``None``: the loop's
    own press. ``step(x0, ref, plant_params, u_prev) -> (losses, features)`` replaces the default body of a step
    (zero_grad, forward, backward, optimizer step). ``noise_sampler(B, T)``: called once per batch, returns that batch's
    ``(process_noise, meas_noise)``, either of which may be ``None`` (for example ``lambda B, T: device_noise(B, T, p_std,
    m_std, device, generator)``); with it a ``step`` is called with ``process_noise=`` and ``meas_noise=`` as well. Returns ``(mean loss per model over the batches, {"cost": (M, sum of
    the batches' B), "metrics": the last batch's})``."""
    if press_loss.loop is not bank_loop:
        raise ValueError("train_on_press: press_loss was built on another loop than bank_loop")
    bank = getattr(bank_loop, "bank", None)
    if hasattr(bank, "train"):
        bank.train()
    costs, total, n_batches, metrics = [], None, 0, None
    for x0, ref, *more in batches:
        u_prev = more[0] if more else None
        plant = None if plant_sampler is None else plant_sampler(x0.shape[-2])
        noise = {}
        if noise_sampler is not None:
            noise["process_noise"], noise["meas_noise"] = noise_sampler(x0.shape[-2], ref.shape[-1])
        if step is not None:
            losses, f = step(x0, ref, plant, u_prev, **noise)
        else:
            optimizer.zero_grad()
            losses, f = press_loss.forward(x0, ref, plant_params=plant, u_prev=u_prev, **noise)
            losses.sum().backward()
            optimizer.step()
        losses = losses.detach()
        costs.append(f["cost"])
        metrics = f.get("metrics")
        total = losses if total is None else total + losses
        n_batches += 1
    M = press_loss.n_models
    avg = (total / n_batches).tolist() if n_batches else [0.0] * M
    return avg, {"cost": torch.cat(costs, dim=1) if costs else torch.empty(M, 0), "metrics": metrics}
