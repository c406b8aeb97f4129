"""The TSRU recurrent unit on the GPU: the kernels of libdvdx_tsru.so against the float64 restatement and its derived bounds
(tests/tsru_ref.py) on the stored operands, the layer against the end-to-end restatement, and a rnn="tsru" Generator / Trainer
through a step, exact resume, prediction and the reports."""
import argparse
import functools
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tsru_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
OUTS = ("h", "da_c", "da_u", "dtheta_raw", "dh_prev")


def _fn():
    from dvd_gan_amd import functional as Fn
    return Fn


_GRU_BEFORE = []


def test_default_path_baseline_before_the_library_is_used():
    """The first test of the module: the losses of a default (ConvGRU) Trainer's first step, taken before anything here has
    loaded libdvdx_tsru.so; test_the_default_path_is_where_it_was, the last one, compares."""
    from dvd_gan_amd import lib as L
    assert "tsru" not in L._handles
    _GRU_BEFORE.extend(_gru_losses())
    assert "tsru" not in L._handles                      # the default path does not touch the extension
    assert len(_GRU_BEFORE) == 6 and all(math.isfinite(v) for v in _GRU_BEFORE)


def _device_step(c, with_hc=True):
    """One forward and one backward launch on the case's operands -> dict of device results (h_c and the gradient tensors whole)."""
    Fn = _fn()
    dtype, d = c["dtype"], c["d"]
    dev = {k: v.to(DEV) for k, v in c.items() if torch.is_tensor(v)}
    B, H, W, C = dev["h_prev"].shape
    h = torch.full((B, H, W, C), float("nan"), device=DEV)
    h_c = torch.full((B, H, W, C), float("nan"), dtype=dtype, device=DEV) if with_hc else None
    Fn.tsru_forward(dev["h_prev"], dev["a"], c["off_c"], c["off_u"], dev["theta_raw"], d, h, h_c)
    da = torch.zeros_like(dev["a"])
    dth = torch.zeros(B, H, W, 8, dtype=dtype, device=DEV)
    dhp = torch.full((B, H, W, C), float("nan"), device=DEV)
    ws = torch.empty(B * H * W * (C + 2), device=DEV)
    Fn.tsru_backward(dev["dh"], None, dev["h_prev"], dev["a"], c["off_c"], c["off_u"], dev["theta_raw"], d, da, c["off_c"], c["off_u"],
                     dth, dev["addend"], dhp, ws)
    torch.cuda.synchronize()
    return {"h": h, "h_c": h_c, "da": da, "dth": dth, "dh_prev": dhp,
            "da_c": da[..., c["off_c"]:c["off_c"] + C], "da_u": da[..., c["off_u"]:c["off_u"] + C], "dtheta_raw": dth[..., :2]}


@functools.lru_cache(maxsize=None)
def _case(case, dtype):
    """(inputs, float64 reference with bounds, device results) of a kernel case: computed once, shared, never changed."""
    c = R.make_case(*case, dtype)
    ref = R.step64(c["h_prev"], c["a"], c["off_c"], c["off_u"], c["theta_raw"], c["d"], dtype, dh=c["dh"], addend=c["addend"])
    return c, ref, _device_step(c)


def _pure_warp(case, dtype, theta_raw=None):
    """The case with u = 1 and c = 0 exactly (sigmoid(40) rounds to 1 in either mode, relu(-1) = 0): h = fmaf(1, warped - 0, 0) is
    the warped state itself, g = dh, and the unit is the linear map whose transpose the backward pass returns."""
    c = dict(R.make_case(*case, dtype))
    a = torch.zeros_like(c["a"])
    C = case[3]
    a[..., c["off_c"]:c["off_c"] + C] = -1.0
    a[..., c["off_u"]:c["off_u"] + C] = 40.0
    c["a"] = a
    c["addend"] = torch.zeros_like(c["addend"])
    if theta_raw is not None:
        c["theta_raw"] = theta_raw
    return c


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", R.CASES)
def test_step_within_the_derived_bounds(case, dtype):
    c, ref, out = _case(case, dtype)
    worst = {}
    for name in OUTS:
        want, bound = ref[name]
        store = dtype if name in ("da_c", "da_u", "dtheta_raw") else torch.float32
        assert out[name].dtype == store
        worst[name] = R.ratio(out[name].cpu(), want, bound, store)
        print(f"MEASURED {case} {dtype} {name}: |out - ref| / bound = {worst[name]:.3e}")
    worst["h_c"] = R.ratio(out["h_c"].cpu(), ref["h"][0], ref["h"][1], dtype)
    assert all(v <= 1.0 for v in worst.values()), worst
    # the copy is the rounded state, and nothing outside the two windows of `da` or the two columns of dtheta_raw was written
    assert torch.equal(out["h_c"], out["h"].to(dtype))
    C = case[3]
    assert float(out["da"][..., :c["off_c"]].abs().max()) == 0.0 and float(out["dth"][..., 2:].abs().max()) == 0.0
    assert out["da"].shape[-1] == c["off_u"] + C


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", R.CASES)
def test_zero_flow_moves_bits(case, dtype):
    B, H, W, C, d = case
    c = _pure_warp(case, dtype, torch.zeros(B, H, W, 2))
    out = _device_step(c)
    assert torch.equal(R.bits(out["h"].cpu()), R.bits(c["h_prev"]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [k for k in R.CASES if float(k[4]).is_integer()])
def test_integer_displacements_are_shifts(case, dtype):
    """tanh(+-20) rounds to +-1 in either mode, so theta is -d, 0 or d exactly on each axis: bilinear reduces to a shift by whole
    pixels, inside the frame and across its border (at 5 x 7 with d = 8 every shifted pixel is outside)."""
    B, H, W, C, d = case
    gen = torch.Generator().manual_seed(5)
    sign = torch.randint(-1, 2, (B, H, W, 2), generator=gen)
    c = _pure_warp(case, dtype, sign.float() * 20.0)
    out = _device_step(c)["h"].cpu()
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    sx, sy = xs + sign[..., 0] * int(d), ys + sign[..., 1] * int(d)
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    b = torch.arange(B).view(B, 1, 1)
    want = c["h_prev"][b, sy.clamp(0, H - 1), sx.clamp(0, W - 1)] * inside.unsqueeze(-1)
    assert bool(inside.any()) or max(H, W) <= d
    assert torch.equal(out, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", R.CASES)
def test_adjoint_identity_on_the_device(case, dtype):
    """<warp h, g> = <h, warp^T g> for the device's own results, within the sum of the two bounds."""
    c = _pure_warp(case, dtype)
    ref = R.step64(c["h_prev"], c["a"], c["off_c"], c["off_u"], c["theta_raw"], c["d"], dtype, dh=c["dh"], addend=c["addend"])
    out = _device_step(c)
    hp, g = c["h_prev"].double(), c["dh"].double()
    lhs, rhs = float((out["h"].cpu().double() * g).sum()), float((hp * out["dh_prev"].cpu().double()).sum())
    allowed = float((ref["h"][1] * g.abs()).sum() + (ref["dh_prev"][1] * hp.abs()).sum())
    print(f"MEASURED {case} {dtype} adjoint: |lhs - rhs| = {abs(lhs - rhs):.3e}, allowed {allowed:.3e}")
    assert abs(lhs - rhs) <= allowed


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", R.CASES)
def test_reruns_and_single_samples_are_bit_equal(case, dtype):
    c, _, out = _case(case, dtype)
    again = _device_step(c)
    names = ("h", "h_c", "da", "dth", "dh_prev")
    for name in names:
        assert torch.equal(R.bits(out[name]), R.bits(again[name])), name
    for b in range(case[0]):
        one = _device_step({k: (v[b:b + 1].contiguous() if torch.is_tensor(v) else v) for k, v in c.items()})
        for name in names:
            assert torch.equal(R.bits(one[name][0]), R.bits(out[name][b])), (name, b)


def test_a_refused_call_leaves_its_outputs_untouched():
    Fn = _fn()
    c = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in R.make_case(*R.CASES[0], torch.float32).items()}
    h, da, dth, dhp = (torch.full(s, 7.0, device=DEV) for s in (c["h_prev"].shape, c["a"].shape, (2, 4, 4, 8), c["h_prev"].shape))
    ws = torch.full((2 * 4 * 4 * 10,), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match=r"libdvdx_tsru: .*flow range.* \(code -1\)"):
        Fn.tsru_forward(c["h_prev"], c["a"], c["off_c"], c["off_u"], c["theta_raw"], 9.0, h, None)
    with pytest.raises(RuntimeError, match=r"libdvdx_tsru: .* \(code -2\)"):
        Fn.tsru_forward(c["h_prev"], c["a"], c["off_c"], c["off_u"] + 8, c["theta_raw"], 2.0, h, None)      # window leaves the row
    with pytest.raises(RuntimeError, match=r"libdvdx_tsru: .* \(code -1\)"):
        Fn.tsru_backward(c["dh"], None, c["h_prev"], c["a"], c["off_c"], c["off_u"], c["theta_raw"], 0.0, da, c["off_c"], c["off_u"],
                         dth, None, dhp, ws)
    torch.cuda.synchronize()
    for t in (h, da, dth, dhp, ws):
        assert float(t.min()) == 7.0 and float(t.max()) == 7.0


# ------------------------------------------------------------------ the layer against the end-to-end restatement
RTOL, ATOL = 2e-3, 2e-4          # what __graft_entry__.smoke() uses for exact mode


def _layer_case(S, with_h0, shared_x):
    """ConvTSRU of two layers (3 x 3 and 5 x 5, Cin != C) with a random non-zero flow head, its inputs and upstream gradients.
    The gate weights are three times their orthogonal initialisation and the biases small, so that no ReLU channel is dead on
    these few pixels (a dead channel has exactly zero gradients, and a zero reference shows nothing)."""
    from dvd_gan_amd.gen_net import ConvTSRU
    T, B, cin, hidden, ks, d = 3, 2, 16, [8, 16], [3, 5], 2.0
    torch.manual_seed(100 + S + 2 * with_h0 + shared_x)
    net = ConvTSRU(cin, hidden, ks, 2, flow=d)
    with torch.no_grad():
        for cell in net.cells:
            torch.nn.init.normal_(cell.flow_out.weight, std=0.3)
            torch.nn.init.normal_(cell.flow_out.bias, std=0.3)
            for gate in (cell.update_gate, cell.out_gate, cell.flow_gate):
                gate.weight.mul_(3.0)
                torch.nn.init.normal_(gate.bias, std=0.1)
    x = torch.randn(B if shared_x else T * B, S, S, cin)
    h0 = [torch.randn(B, S, S, c) for c in hidden] if with_h0 else None
    ups = [torch.randn(T * B, S, S, c) for c in hidden]
    return net, x, h0, ups, T, d


def _layer_ref(net, x, h0, ups, T, d, shared_x):
    """Outputs of both layers and the gradients of every leaf by name, by autograd through the float64 restatement."""
    p64 = [{k: v.detach().double().requires_grad_(True) for k, v in cell.named_parameters()} for cell in net.cells]
    x64 = x.double().requires_grad_(True)
    h64 = [h.double().requires_grad_(True) for h in h0] if h0 is not None else None
    outs, y = [], x64
    for i, p in enumerate(p64):
        y = R.layer64(y, p, T, shared_x and i == 0, h64[i] if h0 is not None else None, d)
        outs.append(y)
    leaves = {"x": x64, **{f"cells.{i}.{k}": v for i, p in enumerate(p64) for k, v in p.items()}}
    if h0 is not None:
        leaves.update({f"h0.{i}": h for i, h in enumerate(h64)})
    grads = torch.autograd.grad(sum((o * u.double()).sum() for o, u in zip(outs, ups)), list(leaves.values()))
    return [o.detach() for o in outs], dict(zip(leaves, grads))


@pytest.mark.parametrize("shared_x", [False, True], ids=["per_step_x", "shared_x"])
@pytest.mark.parametrize("with_h0", [False, True], ids=["zero_state", "h0"])
@pytest.mark.parametrize("S", [4, 8])
def test_layer_matches_the_restatement(S, with_h0, shared_x):
    """ConvTSRU.run in exact mode: the outputs and the gradients of every weight, of x and of h0 against autograd through the
    float64 restatement.  A plumbing check at smoke()'s tolerance: the upstream gradient is scaled until every compared
    gradient's reference median is >= 100 atol, so that the tolerance cannot hide a missing term."""
    net, x, h0, ups, T, d = _layer_case(S, with_h0, shared_x)
    want_outs, want = _layer_ref(net, x, h0, ups, T, d, shared_x)
    # the smallest scale that meets the condition: a weight gradient is an fp32 sum of up to T B S S products, its rounding error
    # about 2^-24 of the sum of their magnitudes -- whatever the sum itself cancels to -- and that term must stay below atol
    scale = max(100 * ATOL / float(g.abs().median()) for g in want.values())
    assert math.isfinite(scale) and scale > 0
    net = net.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    hd = [h.to(DEV).requires_grad_(True) for h in h0] if with_h0 else None
    outs = net.run(xd, T, shared_x, hd)
    leaves = {"x": xd, **{f"cells.{k}": v for k, v in net.cells.named_parameters()}}
    if with_h0:
        leaves.update({f"h0.{i}": h for i, h in enumerate(hd)})
    assert set(leaves) == set(want)
    got = torch.autograd.grad(sum((o * (u.to(DEV) * scale)).sum() for o, u in zip(outs, ups)), list(leaves.values()))
    torch.cuda.synchronize()
    for o, w in zip(outs, want_outs):
        np.testing.assert_allclose(o.detach().cpu().double().numpy(), w.numpy(), rtol=RTOL, atol=ATOL)
    got = dict(zip(leaves, got))
    for name, w in want.items():
        g, w = got[name], w * scale
        assert float(w.abs().median()) >= 100 * ATOL * (1 - 1e-9), name
        np.testing.assert_allclose(g.cpu().double().numpy(), w.numpy(), rtol=RTOL, atol=ATOL, err_msg=name)


# ------------------------------------------------------------------ Generator and Trainer
CH, T_, K_, B_, NCLS, ZD, KS = 2, 4, 4, 2, 3, 16, 4


def _seed(s):
    torch.manual_seed(s)
    random.seed(s)
    np.random.seed(s)


def _cfg(folder=None, **over):
    cfg = dict(adv_loss="hinge", z_dim=ZD, g_chn=CH, ds_chn=CH, dt_chn=CH, n_frames=T_, lr_schr="const", total_epoch=1, d_iters=1,
               batch_size=B_, g_lr=5e-5, d_lr=5e-5, beta1=0.0, beta2=0.9, n_class=NCLS, k_sample=KS, n_cond=K_)
    if folder is not None:
        cfg.update(model_save_path=str(folder), version="", log_epoch=0)
    cfg.update(over)
    return argparse.Namespace(**cfg)


def _trainer(folder=None, rnn="tsru", **over):
    from dvd_gan_amd.train_step import Trainer
    return Trainer([], _cfg(folder, **over), device=DEV, compute_dtype=torch.float32, rnn=rnn)


def _clips(steps=4):
    g = torch.Generator().manual_seed(11)
    return [(torch.rand(B_, 3, K_ + T_, 64, 64, generator=g) * 2 - 1, torch.randint(0, NCLS, (B_,), generator=g)) for _ in range(steps)]


def _state(tr):
    """Every tensor a step leaves for the next: weights, buffers (weight_u / v, batch-norm statistics), Adam moments."""
    out = {}
    for (tag, net), (_, opt) in zip(tr._nets(), tr._optimizers()):
        for k, v in net.state_dict().items():
            out[f"{tag}.{k}"] = v.detach().clone()
        for part in ("m", "v"):
            out[f"{tag}.opt.{part}"] = getattr(opt, part).clone()
    return out


def _differing(a, b):
    assert set(a) == set(b)
    return [k for k in a if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
            or not torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8))]


def _run(tr, clips, first, last):
    return [[v.detach().clone() for v in tr.train_step(*clips[s - 1])] for s in range(first, last + 1)]


def _gru_losses():
    _seed(5)
    return [float(v) for step in _run(_trainer(rnn="gru"), _clips(1), 1, 1) for v in step]


@pytest.fixture(scope="module")
def gru_before():
    """The baseline the module's first test took (it is taken here when a test is run alone: then after whatever ran before)."""
    if not _GRU_BEFORE:
        _GRU_BEFORE.extend(_gru_losses())
    return list(_GRU_BEFORE)


@pytest.fixture(scope="module")
def straight(gru_before, tmp_path_factory):
    """Four uninterrupted rnn="tsru" steps from seed 3 -> (losses of every step, the state they leave)."""
    _seed(3)
    tr = _trainer(tmp_path_factory.mktemp("straight"))
    losses = _run(tr, _clips(), 1, 4)
    return losses, _state(tr)


def test_tsru_step_is_finite_and_reproducible(straight, tmp_path):
    losses, state = straight
    assert all(len(step) == 6 and all(math.isfinite(float(v)) for v in step) for step in losses)
    _seed(3)
    tr = _trainer(tmp_path)
    assert tr.G.rnn == "tsru" and not [k for k in tr.G.state_dict() if "reset_gate" in k]
    again = _run(tr, _clips(), 1, 4)
    assert all(torch.equal(a, b) for sa, sb in zip(losses, again) for a, b in zip(sa, sb))
    bad = _differing(state, _state(tr))
    assert not bad, bad[:10]
    heads = [k for k in state if k.startswith("G.") and k.endswith("flow_out.weight")]
    assert len(heads) == 12 and all(float(state[k].abs().max()) > 0 for k in heads)          # the flow heads left zero


def test_exact_resume(straight, tmp_path):
    want_losses, want = straight
    _seed(3)
    tr = _trainer(tmp_path)
    clips = _clips()
    _run(tr, clips, 1, 2)
    tr.save_state(2, wait=True)
    tr.close_state()
    del tr
    _seed(1234); torch.rand(7); random.random(); np.random.rand()
    fresh = _trainer(tmp_path)
    assert fresh.load_state(os.path.join(str(tmp_path), "2_state.pt")) == []
    got_losses = _run(fresh, clips, 3, 4)
    assert all(torch.equal(a, b) for sa, sb in zip(want_losses[2:], got_losses) for a, b in zip(sa, sb))
    bad = _differing(want, _state(fresh))
    assert not bad, bad[:10]
    assert [k for k in want if k.endswith("weight_u")] and [k for k in want if k.endswith("flow_out.weight")]
    # the other unit's Trainer refuses the file by the first tensor it misses
    with pytest.raises(ValueError, match=r"^net\.G\.conv\.0\.cells\.0\.reset_gate\.weight: the state holds None"):
        _trainer(tmp_path, rnn="gru").load_state(os.path.join(str(tmp_path), "2_state.pt"))


@pytest.mark.parametrize("grad", [False, True], ids=["inference", "training"])
def test_at_initialisation_the_warp_is_the_identity(gru_before, grad):
    """flow_out = 0: the generator's output equals, to the bit, that of the same generator whose host code bypasses the warp (no
    flow head is run and the unit is handed a zero flow, for which the kernel moves h_{t-1}'s bits: test_zero_flow_moves_bits)."""
    from dvd_gan_amd.gen_net import Generator
    Fn = _fn()
    outs = []
    g = torch.Generator().manual_seed(17)
    z, cls = torch.randn(B_, ZD, generator=g).to(DEV), torch.randint(0, NCLS, (B_,), generator=g).to(DEV)
    cond = (torch.rand(B_, K_, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    for bypass in (False, True):
        _seed(23)
        G = Generator(ZD, 4, NCLS, CH, T_, compute_dtype=torch.float32, n_cond=K_, rnn="tsru").to(DEV)
        try:
            Fn.TSRU_BYPASS_WARP = bypass
            with torch.set_grad_enabled(grad):
                outs.append(G(z, cls, cond=cond).detach().clone())
        finally:
            Fn.TSRU_BYPASS_WARP = False
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0
    assert torch.equal(R.bits(outs[0]), R.bits(outs[1]))


def test_prediction_and_reports_leave_no_trace(straight, tmp_path):
    _seed(3)
    tr = _trainer(tmp_path)
    clips = _clips()
    _run(tr, clips, 1, 1)
    before = _state(tr)
    real, labels = clips[1]
    cond = real[:, :, :K_].permute(0, 2, 1, 3, 4).contiguous()
    roll = tr.rollout(cond, labels, 2 * T_ + 1)
    assert tuple(roll.shape) == (B_, 2 * T_ + 1, 3, 64, 64) and bool(torch.isfinite(roll).all())
    assert float(roll.min()) >= 0.0 and float(roll.max()) <= 1.0
    res = tr.evaluate_prediction(real, labels, n_samples=2)
    assert res["psnr"].shape == (T_,) and np.isfinite(res["psnr"]).all() and np.isfinite(res["ssim"]).all()
    bad = _differing(before, _state(tr))
    assert not bad, bad[:10]
    rep = tr.sv_report(iters=4, reset=True)
    rows = [e for e in rep["G"] if ".flow_out." in e["name"] or ".flow_gate." in e["name"]]
    assert len(rows) == 24
    for tag in ("G", "Ds", "Dt"):
        for e in rep[tag]:
            vals = list(e["sv"]) + list(e["res"]) + [e["stable_rank"]] + ([e["sn_sigma"]] if e["sn_sigma"] is not None else [])
            assert all(math.isfinite(v) for v in vals), (tag, e["name"], vals)
    bad = _differing(before, _state(tr))
    assert not bad, bad[:10]
    # an all-zero matrix reports zeros: a fresh generator's flow heads
    _seed(9)
    zero = _trainer(tmp_path).sv_report(iters=2, reset=True)["G"]
    heads = [e for e in zero if e["name"].endswith("flow_out.weight")]
    assert len(heads) == 12
    for e in heads:
        assert all(v == 0.0 for v in e["sv"]) and all(v == 0.0 for v in e["res"]) and e["stable_rank"] == 0.0, e


def test_the_default_path_is_where_it_was(gru_before, straight):
    """A rnn="gru" Trainer built after everything above yields the losses of the one built before: the new library leaves
    nothing behind in shared state."""
    assert _gru_losses() == gru_before
    assert all(math.isfinite(v) for v in gru_before) and len(gru_before) == 6
