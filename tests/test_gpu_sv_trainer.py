"""The Trainer's singular-value monitoring (config.sv_log, Trainer.sv_report, Trainer.sv_history): it changes nothing a step
computes, reports exactly the trainable tensors with dim() >= 2, its numbers stand against the fp64 SVD of the host copies within
their own residuals, the ring keeps one row per logged step and wraps.  The smallest widths of the other trainer tests."""
import argparse
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CH, T, K, NCLS, ZD = 2, 8, 4, 3, 16
S = 64


def _seed(s):
    torch.manual_seed(s)
    random.seed(s)
    np.random.seed(s)


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).clone()


def _trainer(B=2, **over):
    from dvd_gan_amd.train_step import Trainer
    cfg = dict(adv_loss="hinge", z_dim=ZD, g_chn=CH, ds_chn=CH, dt_chn=CH, n_frames=T, lr_schr="const", total_epoch=1, d_iters=1,
               batch_size=B, g_lr=2e-3, d_lr=2e-3, beta1=0.0, beta2=0.9, n_class=NCLS, k_sample=K, log_epoch=0)
    cfg.update(over)
    return Trainer([], argparse.Namespace(**cfg), device=DEV, compute_dtype=torch.float32)


def _clips(B, steps, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 3, T, S, S, generator=g) * 2 - 1, torch.randint(0, NCLS, (B,), generator=g)) for _ in range(steps)]


def _everything(tr):
    """Every bit a step may move: the networks' state_dict entries (weights, weight_u / weight_v, batch-norm statistics), the
    optimizers' flat weights and moments, the default generators."""
    out = {}
    for tag, net in (("G", tr.G), ("Ds", tr.D_s), ("Dt", tr.D_t)):
        for k, v in net.state_dict().items():
            out[f"{tag}.{k}"] = _bits(v)
    for tag, opt in tr._optimizers():
        for name in ("flat", "m", "v"):
            out[f"opt.{tag}.{name}"] = _bits(getattr(opt, name))
        out[f"opt.{tag}.t"] = torch.tensor([int(opt.t)])
    out["rng.cpu"] = torch.get_rng_state().clone()
    out["rng.cuda"] = torch.cuda.get_rng_state(DEV).clone()
    return out


def _run(steps, report_before=False, **over):
    _seed(5)
    tr = _trainer(**over)
    if report_before:
        tr.sv_report()
    losses = []
    for clips, labels in _clips(2, steps):
        losses.append(torch.stack([v.detach().double() for v in tr.train_step(clips, labels)]).cpu())
    torch.cuda.synchronize()
    return tr, losses, _everything(tr)


@pytest.fixture(scope="module")
def plain():
    out = _run(2)
    assert out[0]._sv is None and out[0].sv_history() is None              # off: no table, no workspace, no launch
    return out


def _same(a, b):
    (_, la, sa), (_, lb, sb) = a, b
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(la, lb))
    assert sorted(sa) == sorted(sb)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key


def test_logging_every_step_changes_nothing(plain):
    logged = _run(2, sv_log=1)
    _same(plain, logged)
    hist = logged[0].sv_history()
    assert hist["steps"] == [1, 2] and tuple(hist["G"]["sv"].shape)[0] == 2


def test_report_on_demand_changes_nothing(plain):
    """sv_log = 0: sv_report() builds the monitors at first use, and the steps after it are those of a Trainer that never called it."""
    _same(plain, _run(2, report_before=True))


def _matrices(net):
    return {n: p for n, p in net.named_parameters() if p.requires_grad and p.dim() >= 2}


def test_report_contents(plain):
    tr = plain[0]
    before = _everything(tr)
    rep = tr.sv_report(iters=32)
    after = _everything(tr)
    assert all(torch.equal(before[key], after[key]) for key in before)
    assert sorted(rep) == ["Ds", "Dt", "G"]
    n_sn = 0
    for tag, net in (("G", tr.G), ("Ds", tr.D_s), ("Dt", tr.D_t)):
        want = _matrices(net)
        assert [e["name"] for e in rep[tag]] == list(want) and set(want) <= set(net.state_dict())
        prm = dict(net.named_parameters())
        for e in rep[tag]:
            p = want[e["name"]]
            assert e["shape"] == tuple(p.shape) and len(e["sv"]) == 3 == len(e["res"])
            W = p.detach().cpu().double().reshape(p.shape[0], -1)
            truth = torch.linalg.svdvals(W).numpy()
            sv, res = np.array(e["sv"]), np.array(e["res"])
            assert not np.isnan(sv).any() and not np.isnan(res).any() and np.all(np.diff(sv) <= 0), e
            gap = np.abs(sv[:, None] - np.concatenate([truth, [0.0]])[None, :]).min(1)
            assert np.all(gap <= res + 1e-9 * sv[0]), (e, gap)
            assert np.all(sv[:len(truth)] <= truth[:3] * (1 + 1e-9)) and np.all(sv[len(truth):] == 0.0)
            assert abs(e["stable_rank"] - float((W ** 2).sum()) / sv[0] ** 2) <= 1e-9 * e["stable_rank"]
            if e["name"].endswith("weight_bar"):
                stem = e["name"][:-len("weight_bar")]
                u, v = prm[stem + "weight_u"].detach().cpu().double(), prm[stem + "weight_v"].detach().cpu().double()
                sn = float(u @ W @ v)
                assert abs(e["sn_sigma"] - sn) <= 1e-12 * abs(sn), e
                n_sn += 1
            else:
                assert e["sn_sigma"] is None
    assert n_sn > 10
    # a second report continues from the blocks the first left (warm start): the values do not fall
    again = tr.sv_report(iters=1)
    for tag in rep:
        for a, b in zip(rep[tag], again[tag]):
            assert all(y >= x * (1 - 1e-12) for x, y in zip(a["sv"], b["sv"])), (a, b)
    # reset=True: the seeded start blocks again -- the same numbers as a fresh Trainer's monitors on the same weights
    cold, cold2 = tr.sv_report(iters=4, reset=True), tr.sv_report(iters=4, reset=True)
    assert all(str(a) == str(b) for tag in cold for a, b in zip(cold[tag], cold2[tag]))


def test_history_keeps_one_row_per_logged_step_and_wraps():
    tr, _, _ = _run(3, sv_log=1, sv_log_rows=2, sv_iters=2)
    hist = tr.sv_history()
    assert hist["steps"] == [2, 3]
    n = len(_matrices(tr.G))
    assert tuple(hist["G"]["sv"].shape) == (2, n, 3) == tuple(hist["G"]["res"].shape) and tuple(hist["G"]["fro2"].shape) == (2, n)
    assert hist["G"]["names"] == list(_matrices(tr.G))
    # the newest row is the state the monitors are in: a report without further iterations... needs none -- compare with it
    ring = {tag: tr._sv[tag].ring.cpu() for tag in ("G", "Ds", "Dt")}
    for tag in ring:
        assert torch.equal(hist[tag]["sv"][0], ring[tag][1, :, :3]) and torch.equal(hist[tag]["sv"][1], ring[tag][0, :, :3])
        assert bool((hist[tag]["fro2"] > 0).all())
    # the weights moved between the rows: so did the Frobenius norms
    assert not torch.equal(hist["G"]["fro2"][0], hist["G"]["fro2"][1])
    # every second step only
    tr2, _, _ = _run(3, sv_log=2)
    assert tr2.sv_history()["steps"] == [2]
