"""The device-resident loss scaler without a device: the update rule's restatement pinned to torch's op, the checkpoint format,
the refusals that happen on the host, and the three new symbols of the C ABI."""
import ctypes
import os
import re

import pytest
import torch

import loss_scaler_util as U
from ance_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ance_lamb_step_scaled", "ance_adamw_step_scaled", "ance_loss_scale_update")


def test_update_rule_is_torchs_op_bit_for_bit():
    """loss_scaler_util.update_rule against torch._amp_update_scale_ on CPU tensors over the whole table: the fp32 bits of the scale
    and the tracker."""
    table = U.cases()
    assert len(table) == 72
    seen = set()
    for scale, tracker, flag, gf, bf, interval in table:
        s = torch.tensor([scale], dtype=torch.float32)
        t = torch.tensor([tracker], dtype=torch.int32)
        f = torch.tensor([flag], dtype=torch.float32)
        torch._amp_update_scale_(s, t, f, gf, bf, interval)
        want_s, want_t = U.update_rule(scale, tracker, flag, gf, bf, interval)
        assert (U.bits32(want_s), want_t) == (U.bits32(s.item()), t.item()), (scale, tracker, flag, gf, bf, interval)
        seen.add("back" if want_s < scale else "grow" if want_s > scale else "keep")
    assert seen == {"back", "grow", "keep"}
    # the table holds what it is meant to hold: a growth that would overflow keeps the scale and restarts the tracker
    assert U.update_rule(2.0 ** 127, 4, 0.0, 2.0, 0.5, 5) == (2.0 ** 127, 0)
    assert U.update_rule(65536.0, 3, 0.0, 2.0, 0.5, 5) == (65536.0, 4)
    assert U.update_rule(65536.0, 4, U.NAN, 2.0, 0.5, 5) == (32768.0, 0)


def test_schedule_of_the_known_trajectory():
    """The schedule the GPU trajectory test asserts, from the rule: overflows at steps 1, 2 and 6 of ten, interval 2."""
    scales, tracker = U.schedule(65536.0, (1, 2, 6), 10)
    assert scales == [2.0 ** e for e in (16, 15, 14, 14, 15, 15, 14, 14, 15, 15)] and tracker == 1


def test_state_dict_moves_between_the_two_classes():
    from ance_amd.optim import LossScaler
    ours = LossScaler(init_scale=3.0, growth_factor=1.1, backoff_factor=0.3, growth_interval=7)
    sd = ours.state_dict()
    assert sd == {"scale": 3.0, "growth_factor": 1.1, "backoff_factor": 0.3, "growth_interval": 7, "_growth_tracker": 0}
    theirs = torch.amp.GradScaler("cpu")
    theirs.load_state_dict(sd)
    assert theirs.state_dict() == sd
    theirs_sd = dict(torch.amp.GradScaler("cpu", init_scale=1024.0, growth_interval=11).state_dict(), _growth_tracker=5)
    back = LossScaler()
    back.load_state_dict(theirs_sd)
    assert back.state_dict() == theirs_sd and back.get_scale() == 1024.0 and back._get_growth_tracker() == 5
    assert sorted(sd) == sorted(torch.amp.GradScaler("cpu").state_dict())
    with pytest.raises(RuntimeError, match="empty"):
        back.load_state_dict({})


def test_disabled_scaler_passes_through():
    from ance_amd.optim import LossScaler
    off = LossScaler(enabled=False)
    x = torch.ones(3)
    assert off.scale(x) is x and off.scale([x, x])[1] is x
    assert off.get_scale() == 1.0 and off.state_dict() == {} and not off.is_enabled()
    p = torch.nn.Parameter(torch.ones(2))
    p.grad = torch.ones(2)
    sgd = torch.optim.SGD([p], lr=0.5)
    off.step(sgd)   # any optimizer: step() is called as it is
    off.update()
    off.load_state_dict({"scale": 2.0})
    assert p.detach().tolist() == [0.5, 0.5]


def test_refusals_on_the_host():
    from ance_amd.optim import AdamW, Lamb, LossScaler
    for kw in (dict(init_scale=0.0), dict(init_scale=float("inf")), dict(growth_factor=-2.0), dict(growth_factor=float("nan")),
               dict(backoff_factor=0.0), dict(backoff_factor="x"), dict(growth_interval=0), dict(growth_interval=2.5)):
        with pytest.raises(ValueError):
            LossScaler(**kw)
    scaler = LossScaler()
    p = torch.nn.Parameter(torch.ones(2))
    sgd = torch.optim.SGD([p], lr=0.5)
    with pytest.raises(TypeError, match=r"torch\.optim\.sgd\.SGD"):
        scaler.step(sgd)
    for Opt in (Lamb, AdamW):
        opt = Opt([p])
        with pytest.raises(RuntimeError, match="fused clip .* already works on the unscaled gradients"):
            scaler.unscale_(opt)
        with pytest.raises(RuntimeError, match="no parameter with a gradient"):
            scaler.step(opt)
        with pytest.raises(RuntimeError, match="Closure"):
            scaler.step(opt, lambda: None)
        opt.grad_scale = torch.ones(1)
        with pytest.raises(RuntimeError, match="another scaler"):
            scaler.step(opt)
        assert getattr(opt, "_loss_scaler", None) is None   # nothing of the scaler is left on a refused optimizer
    with pytest.raises(_lib.AnceLibraryError, match="HIP device"):
        scaler.scale(torch.ones(1))
    with pytest.raises(ValueError):
        scaler.scale(3.0)
    with pytest.raises(RuntimeError, match="no scale"):
        scaler.update()


def _prototype(name):
    src = open(os.path.join(ROOT, "include", "ance_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_binding_and_library_agree_on_the_new_symbols():
    L = _lib.lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    ctype_of = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double,
                "size_t": ctypes.c_size_t}
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        res, args = _lib.SYMBOLS[name]
        declared = _prototype(name)
        assert res is ctypes.c_int and len(args) == len(declared), name
        for a, d in zip(args, declared):
            want = ctypes.c_void_p if "*" in d else ctype_of[d.split()[0]]
            assert a is want, (name, d)
    # the planned forms' argument lists, with the flag an output
    assert [d.replace("const ", "") for d in _prototype("ance_lamb_step_scaled")] \
        == [d.replace("const ", "") for d in _prototype("ance_lamb_step_planned")]
    assert [d.replace("const ", "") for d in _prototype("ance_adamw_step_scaled")] \
        == [d.replace("const ", "") for d in _prototype("ance_adamw_step_planned")]
    assert "float *d_found_inf" in _prototype("ance_lamb_step_scaled") and "float *d_found_inf" in _prototype("ance_adamw_step_scaled")
    assert L.ance_abi_version() == _lib.ABI_VERSION == 7


def test_new_entry_points_refuse_before_any_launch():
    """Fake device pointers, never dereferenced: every call below returns on the host."""
    L = _lib.lib()
    fake = [ctypes.c_void_p(0x10000 + 0x100 * i) for i in range(8)]
    big = 1 << 30

    def refused(rc, fn, why):
        msg = L.ance_last_error().decode()
        assert rc == _lib.ANCE_E_INVALID and msg == "%s: invalid argument (%s)" % (fn, why), (rc, msg)

    def lamb(scale=fake[0], flag=fake[1], norm=fake[2], out=fake[4], ws=fake[5], nbytes=big, mgn=1.0, n=7):
        return L.ance_lamb_step_scaled(n, 2, 9, 0, mgn, scale, flag, None, norm, fake[3], out, ws, nbytes, None)

    def adamw(scale=fake[0], flag=fake[1], norm=fake[2], ws=fake[5], nbytes=big, mgn=1.0, n=7):
        return L.ance_adamw_step_scaled(n, 2, 9, 1, mgn, scale, flag, norm, fake[3], ws, nbytes, None)

    for call, fn in ((lamb, "ance_lamb_step_scaled"), (adamw, "ance_adamw_step_scaled")):
        refused(call(scale=None), fn, "null d_grad_scale")
        refused(call(flag=None), fn, "null d_found_inf")
        refused(call(scale=None, mgn=0.0, norm=None), fn, "null d_grad_scale")
        refused(call(flag=None, mgn=0.0, norm=None), fn, "null d_found_inf")
        refused(call(norm=None), fn, "null d_grad_norm")
        refused(call(n=0), fn, "table sizes out of range")
        refused(call(mgn=-1.0), fn, "max_grad_norm not 0 or a positive finite number")
        refused(call(ws=None), fn, "null or unaligned workspace")
        refused(call(nbytes=64), fn, "workspace too small")
    refused(lamb(out=None), "ance_lamb_step_scaled", "null d_out")
    # without the clip the workspace is still the clipped one
    refused(lamb(mgn=0.0, norm=None, nbytes=L.ance_lamb_workspace_bytes(7, 2, 2 * 16384)), "ance_lamb_step_scaled", "workspace too small")
    refused(adamw(mgn=0.0, norm=None, nbytes=L.ance_adamw_workspace_bytes(7, 2, 2 * 16384, 0)), "ance_adamw_step_scaled",
            "workspace too small")

    fn = "ance_loss_scale_update"
    s, t, f = fake[0], fake[1], fake[2]
    refused(L.ance_loss_scale_update(None, t, f, 2.0, 0.5, 2000, None), fn, "null pointer")
    refused(L.ance_loss_scale_update(s, None, f, 2.0, 0.5, 2000, None), fn, "null pointer")
    refused(L.ance_loss_scale_update(s, t, None, 2.0, 0.5, 2000, None), fn, "null pointer")
    refused(L.ance_loss_scale_update(ctypes.c_void_p(0x10002), t, f, 2.0, 0.5, 2000, None), fn, "unaligned pointer")
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        refused(L.ance_loss_scale_update(s, t, f, bad, 0.5, 2000, None), fn, "growth_factor not a positive finite number")
        refused(L.ance_loss_scale_update(s, t, f, 2.0, bad, 2000, None), fn, "backoff_factor not a positive finite number")
    for bad in (0, -5):
        refused(L.ance_loss_scale_update(s, t, f, 2.0, 0.5, bad, None), fn, "growth_interval < 1")
