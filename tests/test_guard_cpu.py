"""CPU checks of the gradient guard (dvd_grad_guard / dvd_adam_guard_step, optim.FlatAdam(clip_norm, skip_nonfinite, norm_log),
Trainer config g_clip_norm / d_clip_norm / skip_nonfinite / grad_log): every refusal that returns before a launch, the workspace
size, the "off allocates nothing" rule, the validation of the Python layers and hipcc's resource report of the new kernels.
Nothing here touches a GPU: the placeholder pointers are never dereferenced."""
import argparse
import ctypes as C
import glob
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
P = C.c_void_p(64)                       # placeholder: non-null, 8-byte aligned, never dereferenced


def _ll(v):
    return C.c_longlong(v)


def _f(v):
    return C.c_float(v)


def _guard(lib, g=P, n=100, max_norm=1.0, skip=1, step=1, ws=P, state=P, ring=None, rows=0):
    return lib.dvd_grad_guard(g, _ll(n), _f(max_norm), skip, _ll(step), ws, state, ring, rows, None)


def _adam(lib, p=P, g=P, m=P, v=P, ema=None, n=100, step=1, decay=0.0, state=P):
    return lib.dvd_adam_guard_step(p, g, m, v, ema, _ll(n), _f(1e-3), _f(0.0), _f(0.9), _f(1e-8), step, _f(decay), state, None)


def test_abi_version_is_unchanged():
    from dvd_gan_amd import lib as L
    assert L.lib().dvd_abi_version() == 13 == L.ABI_VERSION


@pytest.mark.parametrize("kw", [
    dict(g=None), dict(ws=None), dict(state=None), dict(n=0), dict(n=-5), dict(step=0), dict(step=-1),
    dict(max_norm=NAN), dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=-INF),
    dict(rows=-1), dict(ring=P, rows=-1), dict(ring=None, rows=4),
], ids=lambda kw: ",".join(f"{k}={v if not isinstance(v, C.c_void_p) else 'ptr'}" for k, v in kw.items()))
def test_grad_guard_refuses_before_any_launch(kw):
    from dvd_gan_amd import lib as L
    assert _guard(L.lib(), **kw) == -1            # DVD_E_ARG


@pytest.mark.parametrize("kw", [
    dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(state=None), dict(n=0), dict(n=-1), dict(step=0), dict(step=-3),
    dict(ema=P, decay=1.0), dict(ema=P, decay=-0.1), dict(ema=P, decay=NAN), dict(ema=P, decay=1.5),
], ids=lambda kw: ",".join(f"{k}={v if not isinstance(v, C.c_void_p) else 'ptr'}" for k, v in kw.items()))
def test_adam_guard_step_refuses_before_any_launch(kw):
    from dvd_gan_amd import lib as L
    assert _adam(L.lib(), **kw) == -1


def test_workspace_size_is_positive_and_monotone():
    from dvd_gan_amd import kern as K
    sizes = [1, 2, 255, K.GUARD_CH - 1, K.GUARD_CH, K.GUARD_CH + 1, 2 * K.GUARD_CH + 5, 2 ** 20 + 5, 136_700_000, 2 ** 33]
    got = [K.grad_guard_ws_bytes(n) for n in sizes]
    assert all(b > 0 and b % 8 == 0 for b in got), got
    assert got == sorted(got) and got[-1] > got[0]
    # one fp64 partial and one 32-bit count per workgroup of GUARD_CH elements
    assert all(b >= 12 * -(-n // K.GUARD_CH) for n, b in zip(sizes, got))
    assert K.GUARD_CHAIN(1) == K.GUARD_CHAIN(K.GUARD_CH * 1024) < K.GUARD_CHAIN(K.GUARD_CH * 1024 + 1)


def _params():
    return [torch.nn.Parameter(torch.zeros(3, 5)), torch.nn.Parameter(torch.zeros(7))]


def test_flat_adam_without_guard_allocates_nothing():
    from dvd_gan_amd.optim import FlatAdam
    opt = FlatAdam(_params(), 1e-3)
    assert opt.guard is False and opt.clip_norm == 0.0 and opt.skip_nonfinite is False and opt.norm_log == 0
    assert opt.guard_ws is None and opt.guard_state is None and opt.guard_ring is None
    assert opt.grad_norm is None and opt.guard_report() is None
    for kw in (dict(clip_norm=2.0), dict(skip_nonfinite=True), dict(norm_log=3)):
        on = FlatAdam(_params(), 1e-3, **kw)
        assert on.guard is True
        assert on.guard_ws is None and on.guard_state is None and on.guard_ring is None        # until the first step()


@pytest.mark.parametrize("kw", [dict(clip_norm=-1.0), dict(clip_norm=INF), dict(clip_norm=NAN), dict(norm_log=-1)])
def test_flat_adam_rejects_bad_guard_settings(kw):
    from dvd_gan_amd.optim import FlatAdam
    with pytest.raises(ValueError):
        FlatAdam(_params(), 1e-3, **kw)


@pytest.mark.parametrize("kw", [dict(g_clip_norm=-1.0), dict(g_clip_norm=INF), dict(g_clip_norm=NAN), dict(d_clip_norm=-0.5),
                                dict(d_clip_norm=INF), dict(d_clip_norm=NAN), dict(grad_log=-2)])
def test_trainer_rejects_bad_guard_settings(kw):
    """The check sits in Trainer.__init__ ahead of anything that needs a device, like g_ortho's."""
    from dvd_gan_amd.train_step import Trainer
    cfg = argparse.Namespace(adv_loss="hinge", z_dim=16, g_chn=2, ds_chn=2, dt_chn=2, n_frames=8, lr_schr="const", total_epoch=1,
                             d_iters=1, batch_size=2, g_lr=5e-5, d_lr=5e-5, beta1=0.0, beta2=0.9, n_class=3, k_sample=4, **kw)
    with pytest.raises(ValueError, match="clip_norm"):
        Trainer([], cfg, device=torch.device("cpu"), compute_dtype=torch.float32)


def test_guard_kernels_use_no_scratch_memory():
    """hipcc's resource report (build/guard.res, as test_hot_kernels_use_no_scratch_memory reads the others): the norm pass and
    the guarded Adam launch keep everything in registers -- no scratch, no spilled vector registers."""
    path = os.path.join(ROOT, "dvd_gan_amd", "csrc", "build", "guard.res")
    if not glob.glob(path):
        pytest.skip("no build/guard.res: the library was not built by csrc/build.sh in this tree")
    hot = ("grad_sumsq_kernel", "adam_guard_kernel")
    seen, bad = set(), []
    name, rec = None, {}
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name, rec = m.group(1), {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and name:
            rec[m.group(1).strip()] = int(m.group(2))
            if m.group(1).strip() == "VGPRs Spill" and any(h in name for h in hot):
                seen.add(next(h for h in hot if h in name))
                if rec.get("ScratchSize", 0) != 0 and rec.get("SGPRs Spill", 0) == 0 or rec["VGPRs Spill"] != 0:
                    bad.append((name, rec))
    assert seen == set(hot), seen
    assert not bad, bad
