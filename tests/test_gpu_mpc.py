"""GPU: the shooting MPC on the press (fcr_mpc_solve, fcr_mpc_closed_loop) against its fp64 torch
restatement (tests/mpc_ref.py), teacher-forced: every kernel iteration is compared with the restatement's one_iteration
from the kernel's OWN previous (U, lambda), so an accept decision that falls on a tie cannot compound.

Measured on MI355X (largest figures over all cases below): see DESIGN.md §7.17."""
import functools
import os

import numpy as np
import pytest
import torch

import forging_control_amd as fca
import mpc_ref as R
import press_torch as PT

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
dev = lambda a: torch.as_tensor(np.asarray(a, np.float64), device=DEV)
host = lambda t: t.detach().cpu().numpy()


def model_of(form, B):
    """(what PressMPC takes, the (B,28) table the restatement takes)."""
    if form == "none":
        return None, None
    table = PT.three_rows_table(B)
    if form == "row":
        return dev(table[1 % B]), np.tile(table[1 % B], (B, 1))
    return dev(table), table


def setup(B, N, substeps, smooth, mode, form, seed=5):
    """Inputs, the restatement's config with bounds that bind as ``mode`` asks, and the matching PressMPC's kwargs."""
    _, table = model_of(form, B)
    base = R.config(N=N, substeps=substeps, smooth=smooth)
    x0, ref, up, U0, replaced = R.problems(B, N, base, seed, table)
    assert replaced <= 1
    ub, p1, p2 = R.bounds_at_quantiles(x0, ref, up, U0, base, table)
    kw = {}
    if "box" in mode:
        kw["u_bounds"] = ub
    if "hinge" in mode:
        kw.update(p1=p1, p2=p2, w=100.0)
    cfg = R.config(N=N, substeps=substeps, smooth=smooth, **kw)
    U0 = np.clip(U0, cfg["u_lo"], cfg["u_hi"])
    up = np.clip(up, cfg["u_lo"], cfg["u_hi"])
    # the kinks again under the FINAL config: a rolled-out pressure within 1e-6 s_p of a chosen hinge bound counts too
    bad = R.near_kink(R.rollout(R.t64(x0), R.t64(U0), cfg, table), cfg)
    if bad.any():
        x2, r2, u2, U2 = R.draw(B, N, seed + 2000)
        pick = lambda a, b: np.where(bad.reshape((-1,) + (1,) * (a.ndim - 1)), b, a)
        x0, ref = pick(x0, x2), pick(ref, r2)
        up, U0 = pick(up, np.clip(u2, cfg["u_lo"], cfg["u_hi"])), pick(U0, np.clip(U2, cfg["u_lo"], cfg["u_hi"]))
        assert replaced + int(bad.sum()) <= 1
        assert not R.near_kink(R.rollout(R.t64(x0), R.t64(U0), cfg, table), cfg).any()
    return cfg, (x0, ref, up, U0), table


def mpc_of(cfg, K, model, lam0=1e-3):
    return fca.PressMPC(n_horizon=cfg["N"], iters=K, r_u=cfg["r_u"], p1=cfg["p1"], p2=cfg["p2"], p_weight=cfg["w"],
                        p_scale=cfg["s_p"], u_bounds=(cfg["u_lo"], cfg["u_hi"]), lam0=lam0, ts=cfg["ts"],
                        substeps=cfg["substeps"], smooth=cfg["smooth"], model_params=model)


def check_solve(trace, trace_U, lam_end, x0, U_start, u_prev, ref, cfg, table, lam0=1e-3):
    """Teacher-forced comparison of one solve's K iterations (numpy arrays); returns the largest figures and the
    restatement's last iteration."""
    K = trace.shape[1]
    worst, want = {"c": 0.0, "cn": 0.0, "U": 0.0}, None
    assert np.array_equal(trace[:, 0, 2], np.full(len(x0), lam0))
    for i in range(K):
        U_before = U_start if i == 0 else trace_U[:, i - 1]
        got = {"c": trace[:, i, 0], "cn": trace[:, i, 1], "lam_before": trace[:, i, 2], "accept": trace[:, i, 3] != 0,
               "fail": trace[:, i, 4] != 0, "U_before": U_before, "U_after": trace_U[:, i],
               "lam_after": trace[:, i + 1, 2] if i + 1 < K else lam_end}
        want = R.one_iteration(R.t64(x0), R.t64(U_before), R.t64(got["lam_before"]), R.t64(u_prev), R.t64(ref), cfg, table)
        fig, reasons = R.compare_iteration(got, want)
        print(f"  iteration {i}: {fig}, accepted {int(got['accept'].sum())}/{len(x0)}, pivot failures {int(got['fail'].sum())}")
        assert not reasons, (i, reasons)
        worst = {k: max(worst[k], fig[k]) for k in worst}
    return worst, want


SOLVE_CASES = [
    # B, N, K, substeps, smooth, bounds, model
    (1, 1, 1, 4, True, "off", "none"),
    (70, 5, 4, 4, True, "box", "row"),
    (300, 10, 4, 4, True, "box+hinge", "table"),
    (70, 25, 1, 3, False, "hinge", "none"),
    (70, 32, 1, 4, False, "box", "table"),
    (70, 10, 4, 3, True, "off", "row"),
]


@pytest.mark.parametrize("B,N,K,substeps,smooth,mode,form", SOLVE_CASES)
def test_solve_matches_restatement_iteration_by_iteration(B, N, K, substeps, smooth, mode, form):
    cfg, (x0, ref, up, U0), table = setup(B, N, substeps, smooth, mode, form)
    mpc = mpc_of(cfg, K, model_of(form, B)[0])
    out = {k: host(v) for k, v in mpc.solve(dev(x0), dev(ref), dev(up), dev(U0), trace=True).items()}
    if "box" in mode:                                         # each side of the box binds on 5-95 % of the guess
        for side in (U0 <= cfg["u_lo"], U0 >= cfg["u_hi"]):
            assert 0.05 <= side.mean() <= 0.95 or B == 1
    if "hinge" in mode:
        xs = R.rollout(R.t64(x0), R.t64(U0), cfg, table).numpy()
        for col, (lo, hi) in ((2, cfg["p1"]), (3, cfg["p2"])):
            for side in (xs[:, 1:, col] < lo, xs[:, 1:, col] > hi):
                assert 0.05 <= side.mean() <= 0.95
    worst, want = check_solve(out["trace"], out["trace_U"], out["lam"], x0, U0, up, ref, cfg, table)
    print(f"largest figures B={B} N={N} K={K}: {worst}")
    # the outputs are the trace's last state
    assert np.array_equal(out["U"], out["trace_U"][:, -1])
    last = out["trace"][:, -1]
    assert np.array_equal(out["cost"], np.where(last[:, 3] != 0, last[:, 1], last[:, 0]))
    assert np.array_equal(out["accepted"], (out["trace"][:, :, 3] != 0).sum(1))
    info = want[5]
    err = np.abs(out["grad_inf"] - info["grad_inf"].numpy()).max() / info["g"].abs().max().item()
    print(f"grad_inf: {err:.2e} of max|g|")
    assert err <= 1e-9
    # without the trace: the same bits; U0 = None is u_prev repeated
    plain = mpc.solve(dev(x0), dev(ref), dev(up), dev(U0))
    assert all(np.array_equal(host(plain[k]), out[k]) for k in ("U", "cost", "grad_inf", "accepted", "lam"))
    a = mpc.solve(dev(x0), dev(ref), dev(up))
    b = mpc.solve(dev(x0), dev(ref), dev(up), dev(np.repeat(up[:, None], N, 1)))
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_reference_of_shape_B_is_held_over_the_horizon():
    cfg, (x0, ref, up, U0), _ = setup(33, 6, 4, True, "off", "none")
    mpc = mpc_of(cfg, 2, None)
    a = mpc.solve(dev(x0), dev(ref[:, 0]), dev(up))
    b = mpc.solve(dev(x0), dev(np.repeat(ref[:, :1], 6, 1)), dev(up))
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_starting_plan_is_projected_into_the_box():
    """U0 (or u_prev / u_init repeated) outside u_bounds is clipped on load, u_prev itself is not: the call equals the
    one given the clipped plan, bit for bit, and every returned command is inside the box — also in a lane where no
    iteration is accepted (the NaN lane)."""
    cfg, (x0, ref, up, U0), _ = setup(70, 5, 4, True, "box", "none")
    lo, hi = cfg["u_lo"], cfg["u_hi"]
    mpc = mpc_of(cfg, 3, None)
    wide = U0 + np.where(np.arange(70)[:, None] % 2 == 0, 0.5, -0.5)          # every lane has entries outside
    assert ((wide < lo) | (wide > hi)).any(1).all()
    a = mpc.solve(dev(x0), dev(ref), dev(up), dev(wide), trace=True)
    b = mpc.solve(dev(x0), dev(ref), dev(up), dev(np.clip(wide, lo, hi)), trace=True)
    assert all(torch.equal(a[k], b[k]) for k in a)
    out_prev = up + 0.5                                                    # a previous command outside the box
    c = mpc.solve(dev(x0), dev(ref), dev(out_prev))
    d = mpc.solve(dev(x0), dev(ref), dev(out_prev), dev(np.repeat(np.clip(out_prev, lo, hi)[:, None], 5, 1)))
    assert all(torch.equal(c[k], d[k]) for k in c)
    x_bad = x0.copy()
    x_bad[3, 1] = np.nan
    e = mpc.solve(dev(x_bad), dev(ref), dev(up), dev(wide))
    assert int(e["accepted"][3]) == 0
    for r in (a, c, e):
        U = host(r["U"])
        assert (U >= lo).all() and (U <= hi).all()
    T = 4
    loop = mpc.run(dev(x_bad), dev(np.repeat(ref[:, :1], T, 1)), u_init=dev(out_prev), plans=True)
    u = host(loop["u"])
    assert (u >= lo).all() and (u <= hi).all() and (host(loop["accepted"])[3] == 0).all()


def test_nan_lane_leaves_the_others_alone():
    cfg, (x0, ref, up, U0), _ = setup(70, 5, 4, True, "box", "none")
    mpc = mpc_of(cfg, 3, None)
    good = mpc.solve(dev(x0), dev(ref), dev(up), dev(U0))
    x_bad = x0.copy()
    x_bad[17, 2] = np.nan
    bad = mpc.solve(dev(x_bad), dev(ref), dev(up), dev(U0))
    keep = np.arange(70) != 17
    for k in good:
        assert np.array_equal(host(good[k])[keep], host(bad[k])[keep]), k
    assert int(bad["accepted"][17]) == 0 and np.array_equal(host(bad["U"])[17], U0[17])
    T = 3
    r = np.repeat(ref[:, :1], T, 1)
    lg, lb = mpc.run(dev(x0), dev(r)), mpc.run(dev(x_bad), dev(r))
    for k in ("x", "u", "cost", "accepted"):
        assert np.array_equal(host(lg[k])[keep], host(lb[k])[keep]), k


# ------------------------------------------------------------------------------------------------ the closed loop

def loop_inputs(B, T, seed=7):
    rng = np.random.default_rng(seed)
    d = R.trace_mpc()
    rows = d[rng.integers(0, len(d), B)]
    x0 = rows[:, 2:7] * (1 + 0.05 * rng.standard_normal((B, 5)))
    ref = np.repeat(rng.uniform(-0.9, 0.9, (B, 1)), T, 1)
    if T > 2:                                                 # a jump two steps ahead: inside every horizon before it
        ref[:, 2:] = rng.uniform(-0.9, 0.9, (B, 1))
    scale = np.abs(d[:, 2:7]).max(0)
    wn = 0.02 * rng.standard_normal((B, T, 5)) * scale / 1e-3 * 1e-2
    vn = 1e-3 * rng.standard_normal((B, T, 5)) * scale
    return x0, ref, rows[:, 7].copy(), wn, vn


LOOP_CASES = [
    # B, N, K, T, substeps, smooth, noise, preview, plant, model; the first four reach <1, table, off>, <1, table, on>,
    # <0, table, on>, <1, literal, off> (a table for either press runs both as tables)
    (70, 5, 2, 6, 4, True, False, True, "table", "none"),
    (33, 4, 2, 6, 3, True, True, False, "none", "row"),
    (33, 4, 2, 6, 4, False, True, True, "table", "table"),
    (5, 3, 1, 1, 4, True, False, True, "none", "none"),
    # the other four instantiations of mpc_closed_loop_kernel<SMOOTH, table, NOISE>
    (33, 4, 2, 6, 4, True, True, True, "none", "none"),      # <1, literal, on>
    (33, 4, 2, 6, 3, False, False, True, "none", "none"),    # <0, literal, off>
    (9, 3, 1, 1, 4, False, True, False, "none", "none"),     # <0, literal, on>
    (33, 4, 2, 6, 4, False, False, False, "none", "table"),  # <0, table, off>
]


@pytest.mark.parametrize("B,N,K,T,substeps,smooth,noise,preview,plant,model", LOOP_CASES)
def test_closed_loop_step_by_step(B, N, K, T, substeps, smooth, noise, preview, plant, model):
    x0, ref, u_init, wn, vn = loop_inputs(B, T)
    m_arg, m_tab = model_of(model, B)
    p_arg, p_tab = model_of(plant, B)
    if plant == "table" and model == "table":                # a plant that is not the model
        p_tab = np.roll(p_tab, 1, axis=0)
        p_arg = dev(p_tab)
    cfg = R.config(N=N, substeps=substeps, smooth=smooth, u_bounds=(-0.25, 0.25))
    mpc = mpc_of(cfg, K, m_arg)
    kw = dict(process_noise=dev(wn) if noise else None, meas_noise=dev(vn) if noise else None, plant_params=p_arg,
              preview=preview, u_init=dev(u_init))
    out = mpc.run(dev(x0), dev(ref), plans=True, trace=True, **kw)
    o = {k: host(v) for k, v in out.items() if torch.is_tensor(v)}
    assert o["x"].shape == (B, T + 1, 5) and np.array_equal(o["x"][:, 0], x0)
    worst = {"c": 0.0, "cn": 0.0, "U": 0.0}
    for t in range(T):
        print(f" step {t}")
        start = (np.clip(np.repeat(u_init[:, None], N, 1), cfg["u_lo"], cfg["u_hi"]) if t == 0
                 else R.shift_plan(torch.as_tensor(o["plans"][:, t - 1])).numpy())
        u_prev = u_init if t == 0 else o["u"][:, t - 1]
        refs = R.horizon_refs(R.t64(ref), t, N, preview).numpy()
        if T > 2 and t < 2:
            assert (refs != refs[:, :1]).any() == preview        # the jump is inside the horizon iff previewed
        lam_end = np.where(o["trace"][:, t, -1, 3] != 0, np.maximum(o["trace"][:, t, -1, 2] * 0.3, 1e-12),
                           np.minimum(o["trace"][:, t, -1, 2] * 10.0, 1e12))
        w, _ = check_solve(o["trace"][:, t], o["trace_U"][:, t], lam_end, o["x"][:, t], start, u_prev, refs, cfg, m_tab)
        worst = {k: max(worst[k], w[k]) for k in worst}
        assert np.array_equal(o["plans"][:, t], o["trace_U"][:, t, -1])
        assert np.array_equal(o["u"][:, t], o["plans"][:, t, 0])
        assert np.array_equal(o["accepted"][:, t], (o["trace"][:, t, :, 3] != 0).sum(1))
        x_true = o["x"][:, t] - (vn[:, t - 1] if noise and t > 0 else 0.0)
        with torch.no_grad():
            xn = R.plant_step(R.t64(x_true), R.t64(o["u"][:, t]), cfg, p_tab, R.t64(wn[:, t]) if noise else None).numpy()
        xn = xn + (vn[:, t] if noise else 0.0)
        err = (np.abs(o["x"][:, t + 1] - xn).max(0) / np.abs(xn).max(0)).max()
        print(f"  plant step: {err:.2e}")
        assert err <= 1e-12
    print(f"largest figures of the loop: {worst}")
    again = mpc.run(dev(x0), dev(ref), plans=True, trace=True, **kw)
    assert all(torch.equal(out[k], again[k]) for k in ("x", "u", "cost", "grad_inf", "accepted", "plans", "trace", "trace_U"))
    plain = mpc.run(dev(x0), dev(ref), **kw)
    assert all(torch.equal(out[k], plain[k]) for k in ("x", "u", "cost", "grad_inf", "accepted"))
    assert "plans" not in plain and "trace" not in plain


def test_empty_runs():
    mpc = fca.PressMPC(n_horizon=4, iters=2)
    x0 = dev(loop_inputs(3, 1)[0])
    r = mpc.run(x0, torch.zeros(3, 0, dtype=torch.float64, device=DEV))
    assert torch.equal(r["x"][:, 0], x0) and r["u"].shape == (3, 0) and float(r["metrics"]["RMSE"]) == 0.0
    r = mpc.run(x0[:0], torch.zeros(0, 5, dtype=torch.float64, device=DEV))
    assert r["x"].shape == (0, 6, 5)
    s = mpc.solve(x0[:0], torch.zeros(0, dtype=torch.float64, device=DEV), torch.zeros(0, dtype=torch.float64, device=DEV))
    assert s["U"].shape == (0, 4)


# ------------------------------------------------------------------------------------------------ metrics, dataset, behaviour

@functools.lru_cache(maxsize=None)
def behaviour_run():
    """B = 256, T = 60 around the reference step of the trace fixture at t = 149 -> 150 (0.578 -> -0.295), K = 3."""
    rng = np.random.default_rng(1)
    d = R.trace_mpc()
    i0, B, T = 120, 256, 60
    x0 = d[i0, 2:7] * (1 + 0.02 * rng.standard_normal((B, 5)))
    ref = np.tile(d[i0:i0 + T, 1], (B, 1))
    assert ref[0, 0] != ref[0, -1]
    u_init = float(d[i0 - 1, 7])
    mpc = fca.PressMPC(n_horizon=10, iters=3, p1=(0.0, 32e6), p2=(0.0, 32e6))
    return mpc.run(dev(x0), dev(ref), u_init=u_init), x0, ref, u_init


def test_metrics_match_numpy_on_the_record():
    out, _, ref, _ = behaviour_run()
    x, u, m = host(out["x"]), host(out["u"]), out["metrics"]
    e = x[:, 1:, 1] - ref
    viol = np.max([0.0 - x[:, 1:, 2], x[:, 1:, 2] - 32e6, 0.0 - x[:, 1:, 3], x[:, 1:, 3] - 32e6], 0)
    want = {"MAE": np.abs(e).mean(), "RMSE": np.sqrt((e * e).mean()), "R2": 1 - (e * e).sum() / ((ref - ref.mean()) ** 2).sum(),
            "max_err": np.abs(e).max(), "Command": np.abs(u).mean(), "du_rms": np.sqrt((np.diff(u, axis=1) ** 2).mean()),
            "viol_max": viol.max(), "viol_frac": (viol > 0).mean()}
    for k, v in want.items():
        assert abs(float(m[k]) - v) <= 1e-12 * max(1.0, abs(v)), (k, float(m[k]), v)
    assert np.allclose(host(m["traj"]["MAE"]), np.abs(e).mean(1), rtol=1e-12, atol=0)
    assert np.allclose(host(m["traj"]["max_err"]), np.abs(e).max(1), rtol=1e-12, atol=0)
    r2 = 1 - (e * e).sum(1) / ((ref - ref.mean(1, keepdims=True)) ** 2).sum(1)
    assert np.allclose(host(m["traj"]["R2"]), r2, rtol=1e-10, atol=0)
    assert set(m["traj"]) == {"MAE", "RMSE", "R2", "max_err", "Command", "du_rms", "viol_max"}


def test_dataset_feeds_the_supervised_epoch():
    out, _, ref, _ = behaviour_run()
    X, y = fca.mpc_dataset(out, PT.SCALERS)
    B, T = ref.shape
    assert X.shape == (B * T, 3) and y.shape == (B * T, 1) and X.dtype == y.dtype == torch.float32 and X.is_cuda
    x, u = host(out["x"]), host(out["u"])
    assert np.allclose(host(X[:, 0]), (x[:, :-1, 1] / PT.SCALERS["input"][0]).reshape(-1), rtol=1e-6)
    assert np.allclose(host(X[:, 1]), (x[:, :-1, 4] / PT.SCALERS["input"][1]).reshape(-1), rtol=1e-6)
    assert np.allclose(host(X[:, 2]), (ref / PT.SCALERS["y_dot"]).reshape(-1), rtol=1e-6)
    assert np.allclose(host(y[:, 0]), (u / PT.SCALERS["output"]).reshape(-1), rtol=1e-6)
    model = fca.FNNModel(3, 50, 1, 1).to(DEV)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    loss = fca.supervised.train_epoch(model, opt, X, y, batch_size=256, generator=torch.Generator().manual_seed(0))
    assert np.isfinite(loss)


def test_mpc_tracks_a_reference_step():
    out, x0, ref, u_init = behaviour_run()
    x = host(out["x"])
    rmse = np.sqrt(((x[:, 31:, 1] - ref[:, 30:]) ** 2).mean())
    hold = host(fca.forging_rk4(dev(x0), torch.full(ref.shape, u_init, dtype=torch.float64, device=DEV), smooth=True))
    rmse_hold = np.sqrt(((hold[:, 31:, 1] - ref[:, 30:]) ** 2).mean())
    accepted = (host(out["accepted"])[:, :10] >= 1).mean()
    w = np.load(os.path.join(PT.GOLDEN, "ul_seed_controllers.npz"))
    ctrl = fca.FNNModel(3, 50, 1, 1).to(DEV)
    with torch.no_grad():
        ctrl.fc_inp.weight.copy_(torch.as_tensor(w["W_inp"][0]))
        ctrl.fc_inp.bias.copy_(torch.as_tensor(w["b_inp"][0]))
        ctrl.fc_out.weight.copy_(torch.as_tensor(w["W_out"][0]))
    xn, _ = fca.ClosedLoop(ctrl, PT.SCALERS).run(dev(x0), dev(ref))
    rmse_nn = np.sqrt(((host(xn)[:, 31:, 1] - ref[:, 30:]) ** 2).mean())
    print(f"RMSE over the last 30 steps: MPC {rmse:.4f}, holding u_init {rmse_hold:.4f}, NN controller (seed 0) {rmse_nn:.4f}; "
          f"accepted >= 1 on {accepted:.3f} of the first ten steps; mean cost {float(out['cost'].mean()):.4f}")
    assert rmse < rmse_hold
    assert accepted >= 0.90
