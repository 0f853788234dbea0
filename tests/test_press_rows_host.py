"""CPU: the press rows' entry points share their argument checks (csrc/fcr_press_host.h). One table of faults of the
fields the loop structs begin with goes to fcr_closed_loop_run, fcr_closed_loop_run_bank, fcr_closed_loop_run_bank_press
and fcr_closed_loop_vjp; one table of parameter-table faults to fcr_plant_rk4_press, fcr_closed_loop_run_bank_press,
fcr_plant_rk4_vjp and fcr_closed_loop_vjp. Every call is valid but for the one fault, so each is refused before any
launch, with the same code everywhere and a message that names the entry point called and the bad field."""
import ctypes

import pytest

import forging_control_amd as fca

N = fca._native
FAKE = 4096                                 # a non-NULL, aligned address no refused call ever reads
MAX_HIDDEN = 256                            # closed_loop::kClMaxHidden and press_grad::kMaxHidden (csrc)


def loop_struct(cls, **kw):
    """A struct of `cls` that passes every check (all its pointers FAKE), then `kw`."""
    a = cls()
    a.B, a.T, a.ts, a.substeps, a.smooth, a.ctrl_hidden = 4, 3, 1e-3, 4, 1, 50
    a.in_scale[0] = a.in_scale[1] = a.ref_scale = a.out_scale = 1.0
    for name, ctype in cls._fields_:
        if ctype is ctypes.c_void_p and name not in ("process_noise", "meas_noise", "u_nn", "feas_flag", "press"):
            setattr(a, name, FAKE)
    if cls is N.FcrClosedLoopBank:
        a.n_models, a.p1_hi, a.p2_hi = 2, 32e6, 32e6
    for k, v in kw.items():
        if k == "in_scale0":
            a.in_scale[0] = v
        else:
            setattr(a, k, v)
    return a


def call_loop(name, kw, null=False, table=(FAKE, 0, 28)):
    """Entry point `name` on a valid struct with the fields `kw` (null: on no struct), the *_press / *_vjp ones with
    `table` = (pointer, stride_model, stride_traj); -> (code, message)."""
    lib = N.load()
    cls = {"fcr_closed_loop_run": N.FcrClosedLoop, "fcr_closed_loop_vjp": N.FcrClosedLoopGrad}.get(name, N.FcrClosedLoopBank)
    if name == "fcr_closed_loop_vjp":
        kw = dict(kw, press=table[0], stride_traj=table[2])
    a = None if null else ctypes.byref(loop_struct(cls, **kw))
    if name == "fcr_closed_loop_run_bank_press":
        rc = lib.fcr_closed_loop_run_bank_press(a, table[0], table[1], table[2], None, None)
    elif name == "fcr_closed_loop_vjp":
        rc = lib.fcr_closed_loop_vjp(a, FAKE, 1 << 30, None)
    else:
        rc = getattr(lib, name)(a, None)
    return rc, lib.fcr_last_error().decode()


LOOPS = ("fcr_closed_loop_run", "fcr_closed_loop_run_bank", "fcr_closed_loop_run_bank_press", "fcr_closed_loop_vjp")
LOOP_FAULTS = [
    (dict(B=-1), -1, "B=-1"), (dict(T=-2), -1, "T=-2"), (dict(substeps=0), -1, "substeps=0"), (dict(ts=0.0), -1, "ts=0"),
    (dict(ts=-1.0), -1, "ts=-1"), (dict(smooth=2), -1, "smooth=2"), (dict(ctrl_hidden=0), -4, "ctrl_hidden=0"),
    (dict(ctrl_hidden=MAX_HIDDEN + 1), -4, f"ctrl_hidden={MAX_HIDDEN + 1}"), (dict(ref_scale=0.0), -1, "scales must be positive"),
    (dict(in_scale0=0.0), -1, "scales must be positive"), (dict(out_scale=float("nan")), -1, "scales must be positive"),
]


@pytest.mark.parametrize("name", LOOPS)
@pytest.mark.parametrize("kw,code,word", LOOP_FAULTS, ids=[w for _, _, w in LOOP_FAULTS[:8]] + ["ref_scale=0", "in_scale=0", "out_scale=nan"])
def test_a_common_fault_is_refused_alike_by_every_loop(name, kw, code, word):
    rc, msg = call_loop(name, kw)
    assert rc == code and msg.startswith(name + ":") and word in msg, (rc, msg)


@pytest.mark.parametrize("name", LOOPS)
def test_a_null_struct_is_refused_alike_by_every_loop(name):
    rc, msg = call_loop(name, {}, null=True)
    assert rc == -1 and msg.startswith(name + ":") and "args is NULL" in msg, (rc, msg)


@pytest.mark.parametrize("name", LOOPS)
def test_the_widest_controller_passes_the_shared_checks(name):
    """ctrl_hidden at the entry point's own maximum with B = 0: every shared check passes and the empty call is a no-op
    (the adjoint's with nothing to zero), so MAX_HIDDEN + 1 above is one above the maximum."""
    empty = dict(B=0, ctrl_hidden=MAX_HIDDEN, g_w_inp=None, g_b_inp=None, g_w_out=None) if name == "fcr_closed_loop_vjp" \
        else dict(B=0, ctrl_hidden=MAX_HIDDEN)
    rc, msg = call_loop(name, empty)
    assert rc == 0, msg


def call_table(name, press, stride_traj):
    """Entry point `name`, valid but for its parameter table; -> (code, message)."""
    lib = N.load()
    if name == "fcr_plant_rk4_press":
        rc = lib.fcr_plant_rk4_press(4, 3, 1e-3, 4, 0, FAKE, FAKE, FAKE, press, stride_traj, None)
    elif name == "fcr_plant_rk4_vjp":
        rc = lib.fcr_plant_rk4_vjp(4, 3, 1e-3, 4, 0, FAKE, FAKE, FAKE, press, stride_traj, FAKE, FAKE, None)
    else:
        return call_loop(name, {}, table=(press, 0, stride_traj))
    return rc, lib.fcr_last_error().decode()


TABLES = ("fcr_plant_rk4_press", "fcr_closed_loop_run_bank_press", "fcr_plant_rk4_vjp", "fcr_closed_loop_vjp")
TABLE_FAULTS = [((FAKE, -28), ("stride is negative", "trajectory -28")), ((FAKE, 27), ("stride_traj=27", "multiple of 28")),
                ((FAKE + 4, 28), ("parameter table must be 8-byte aligned",)), ((None, 28), ("parameter table",))]


@pytest.mark.parametrize("name", TABLES)
@pytest.mark.parametrize("table,words", TABLE_FAULTS, ids=["negative", "27", "misaligned", "stride-without-table"])
def test_a_table_fault_is_refused_alike_by_every_entry_point(name, table, words):
    rc, msg = call_table(name, *table)
    assert rc == -1 and msg.startswith(name + ":") and all(w in msg for w in words), (rc, msg)
