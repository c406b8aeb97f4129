"""The Trainer's balanced consistency regularization (Trainer(d_cr=, d_cr_fake=)): off is the step as it was; on, every
discriminator call of a D iteration takes [transformed | clean] views of the same clips and the penalty's gradient reaches the
discriminators exactly as the CPU oracle computes it, nothing reaches the generator, the frame-conditional clean view holds the raw
context, a resumed run continues bit-equal, and cr_report() reads the statistics.  The smallest widths the discriminators accept
(tests/test_gpu_geom_trainer.py's)."""
import argparse
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CH, T, K, NCLS, ZD = 2, 8, 4, 3, 16
S = 64
AUG = "color,translation,cutout"
E32 = 2.0 ** -24


def _seed(s):
    torch.manual_seed(s)
    random.seed(s)
    np.random.seed(s)


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).clone()


def _trainer(B=2, folder=None, kw=None, **over):
    from dvd_gan_amd.train_step import Trainer
    cfg = dict(adv_loss="hinge", z_dim=ZD, g_chn=CH, ds_chn=CH, dt_chn=CH, n_frames=T, lr_schr="const", total_epoch=1, d_iters=1,
               batch_size=B, g_lr=2e-3, d_lr=2e-3, beta1=0.0, beta2=0.9, n_class=NCLS, k_sample=K, log_epoch=0, d_aug=AUG)
    if folder is not None:
        cfg.update(model_save_path=str(folder), version="")
    cfg.update(over)
    return Trainer([], argparse.Namespace(**cfg), device=DEV, compute_dtype=torch.float32, **(kw or {}))


def _clips(B, steps, seed=11, frames=T):
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, 3, frames, S, S, generator=g) * 2 - 1, torch.randint(0, NCLS, (B,), generator=g)) for _ in range(steps)]


def _flats(tr):
    return [_bits(opt.flat) for _, opt in tr._optimizers()]


def _tables(B, seed):
    """Rows that transform EVERY clip: each group of the policy applies (p = 1), brightness / saturation / contrast, a shift and
    a cutout of a quarter of the frame."""
    from dvd_gan_amd.augment import draw_params
    gen = torch.Generator().manual_seed(seed)
    return {"aug_real": draw_params(B, S, S, AUG, 1.0, gen), "aug_fake": draw_params(B, S, S, AUG, 1.0, gen)}


def _draws(B, seed=3, **tables):
    g = torch.Generator().manual_seed(seed)
    d = {"perm_real": torch.randperm(T, generator=g), "z": torch.randn(B, ZD, generator=g),
         "z_class": torch.randint(0, NCLS, (B,), generator=g), "perm_fake": torch.randperm(T, generator=g)}
    d.update(tables)
    return d


def _watch(tr):
    """Record (input, labels, logits) of every call of the two discriminators and what the generator returns, in order."""
    seen = {"Ds": [], "Dt": [], "G": []}
    for tag, net in (("Ds", tr.D_s), ("Dt", tr.D_t)):
        def forward(*a, _orig=net.forward, _tag=tag, **kw):
            out = _orig(*a, **kw)
            seen[_tag].append((a[0].detach().clone(), a[1].detach().clone(), out.detach().clone()))
            return out
        net.forward = forward
    tr.G.register_forward_hook(lambda m, a, out: seen["G"].append(out.detach().clone()))
    return seen


def _at_adam(tr, record):
    """Call record(tag) right before every Adam launch of D_s / D_t."""
    for tag, opt in (("Ds", tr.ds_optimizer), ("Dt", tr.dt_optimizer)):
        def stepper(tag=tag, orig=opt.step):
            record(tag)
            orig()
        opt.step = stepper


def _ids(draws):
    return draws["perm_real"][:K].sort()[0], draws["perm_fake"][:K].sort()[0]


# ------------------------------------------------------------------ 1. off is the parent
def test_off_is_the_step_without_the_keywords():
    B, runs = 2, []
    for kw in (None, dict(d_cr=0.0), dict(d_cr=0.0, d_cr_fake=0.0)):
        _seed(5)
        tr = _trainer(B, kw=kw, d_aug_p=0.7)
        losses = [[_bits(v) for v in tr.train_step(*c)] for c in _clips(B, 2)]
        torch.cuda.synchronize()
        runs.append((losses, _flats(tr), torch.get_rng_state()))
        assert tr._cr_stats is None and tr.cr_report() is None and tr.d_cr == 0.0 and tr.d_cr_fake == 0.0
    for lb, fb, rb in runs[1:]:
        for step in range(2):
            for a, b in zip(runs[0][0][step], lb[step]):
                assert torch.equal(a, b), step
        for a, b in zip(runs[0][1], fb):
            assert torch.equal(a, b)
        assert torch.equal(runs[0][2], rb)


# ------------------------------------------------------------------ 2. what the discriminators are given
@pytest.mark.parametrize("d_iters", [1, 2])
def test_every_d_call_takes_the_transformed_then_the_clean_views(d_iters):
    from dvd_gan_amd.helpers import sample_k_frames, vid_downsample
    B = 2
    (clips, labels) = _clips(B, 1)[0]
    draws = [_draws(B, seed=3 + i, **_tables(B, 50 + i)) for i in range(d_iters)]
    seen = []
    for kw in (None, dict(d_cr=10.0)):
        _seed(7)
        tr = _trainer(B, kw=kw, d_aug_p=1.0, d_iters=d_iters)
        seen.append(_watch(tr))
        tr.train_step(clips, labels, draws if d_iters > 1 else draws[0])
        torch.cuda.synchronize()
    plain, cr = seen
    assert [len(cr[k]) for k in ("Ds", "Dt", "G")] == [2 * d_iters + 1, 2 * d_iters + 1, d_iters]
    real5 = clips.permute(0, 2, 1, 3, 4).contiguous().to(DEV)
    for it in range(d_iters):
        ids_real, ids_fake = _ids(draws[it])
        fake5 = cr["G"][it]
        assert torch.equal(fake5, plain["G"][it])                         # the generator has not moved between the D iterations
        clean = {"Ds": (sample_k_frames(real5, T, K, ids_real), sample_k_frames(fake5, T, K, ids_fake)),
                 "Dt": (vid_downsample(real5), vid_downsample(fake5))}
        want_labels = (labels, draws[it]["z_class"])
        for tag, n in (("Ds", B), ("Dt", B)):
            for j, what in enumerate(("real", "fake")):
                x, cls, out = cr[tag][2 * it + j]
                x0, cls0, out0 = plain[tag][2 * it + j]
                assert x.shape[0] == 2 * n and tuple(x.shape[1:]) == tuple(x0.shape[1:]) and out.numel() == 2 * out0.numel(), (tag, what)
                assert torch.equal(_bits(x[:n]), _bits(x0)), (tag, what, it, "transformed half")
                assert torch.equal(_bits(x[n:]), _bits(clean[tag][j])), (tag, what, it, "clean half")
                assert not torch.equal(x[:n], x[n:])                      # the rows transform every clip
                assert torch.equal(cls.cpu(), torch.cat([want_labels[j], want_labels[j]])) and torch.equal(cls0.cpu(), want_labels[j])
    # the generator step: n samples, the transformed views, as without the feature
    for tag in ("Ds", "Dt"):
        x, cls, _ = cr[tag][-1]
        x0, cls0, _ = plain[tag][-1]
        assert x.shape == x0.shape and x.shape[0] == B and torch.equal(_bits(x), _bits(x0)) and torch.equal(cls, cls0)


# ------------------------------------------------------------------ 3. gradient parity with the oracle
def _cos(a, b):
    """tests/test_gpu_trainer.py's: 1.0 when both gradients are exactly zero (attention behind gamma = 0), 0.0 when one is."""
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    if float(b.norm()) == 0.0:
        return 1.0 if float(a.norm()) == 0.0 else 0.0
    return float((a * b).sum() / (a.norm() * b.norm() + 1e-300))


def _oracle(O, disc, arrays, calls, adv, weights):
    """The oracle discriminator on the recorded 2n-sample inputs, real then fake (u / v advance per call as on the device) ->
    (adversarial terms, penalties, gradient of their sum, gradient of the adversarial terms alone) per named parameter."""
    sd = O.make_state(arrays)
    outs = [disc(sd, x, cls) for x, cls, _ in calls]
    advs, pens = [], []
    for out, (_, _, flag), w in zip(outs, calls, weights):
        n = out.numel() // 2
        advs.append(O.adv_loss(out[:n], flag, adv))
        pens.append(w * ((out[:n] - out[n:]) ** 2).mean())
    prm = O.trainable(sd)
    keys = list(prm)
    plain = torch.autograd.grad(advs[0] + advs[1], [prm[k] for k in keys], retain_graph=True, allow_unused=True)
    full = torch.autograd.grad(advs[0] + advs[1] + pens[0] + pens[1], [prm[k] for k in keys], allow_unused=True)
    grads = {k: (f.detach(), p.detach()) for k, f, p in zip(keys, full, plain) if f is not None}
    return [float(v.detach()) for v in advs], [float(v.detach()) for v in pens], grads


@pytest.mark.parametrize("adv", ["hinge", "wgan-gp"])
def test_discriminator_gradients_match_the_oracle(adv):
    """Tolerances: the project's exact-mode ones (tests/test_gpu_trainer.py at the reference's initialisation,
    __graft_entry__.smoke): losses and penalties rtol 2e-3 / atol 2e-4, |grad| checksum of every parameter 1e-2 relative (over
    the parameters whose checksum is above 1e-3 of the largest, as there), named-gradient cosine >= 0.9999.  The penalty must
    matter: for each network the oracle's gradient without it has cosine < 0.99 against the one with it for some parameter."""
    from oracle import dvdgan_cpu as O
    B = 2
    _seed(23)
    tr = _trainer(B, kw=dict(d_cr=10.0, d_cr_fake=5.0), adv_loss=adv, d_aug_p=1.0)
    arrays = {tag: {k: v.detach().cpu().clone() for k, v in net.state_dict().items()} for tag, net in (("Ds", tr.D_s), ("Dt", tr.D_t))}
    seen, snaps = _watch(tr), {}
    nets = {"Ds": tr.D_s, "Dt": tr.D_t}
    _at_adam(tr, lambda tag: snaps.setdefault(tag, {k: p.grad.detach().cpu().clone() for k, p in nets[tag].named_parameters()
                                                    if p.grad is not None}))
    (clips, labels), draws = _clips(B, 1)[0], _draws(B, **_tables(B, 61))
    got = [float(v.detach()) for v in tr.train_step(clips, labels, draws)]
    rep = tr.cr_report()
    for i, (tag, disc) in enumerate((("Ds", O.spatial_disc), ("Dt", O.temporal_disc))):
        calls = [(x.cpu(), cls.cpu(), flag) for (x, cls, _), flag in zip(seen[tag][:2], (True, False))]
        advs, pens, grads = _oracle(O, disc, arrays[tag], calls, adv, (10.0, 5.0))
        got_pens = [rep[f"{tag}_real"]["penalty"], rep[f"{tag}_fake"]["penalty"]]
        print(f"[cr] {adv} {tag}: losses {got[2 * i:2 * i + 2]} / {advs}, penalties {got_pens} / {pens}")
        np.testing.assert_allclose(got[2 * i:2 * i + 2], advs, rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(got_pens, pens, rtol=2e-3, atol=2e-4)
        assert min(pens) > 1e-3                                            # both penalties are there to be compared
        keys = list(grads)
        assert keys and set(keys) <= set(snaps[tag])
        ref = np.array([float(grads[k][0].double().abs().sum()) for k in keys])
        dev = np.array([float(snaps[tag][k].double().abs().sum()) for k in keys])
        big = ref > 1e-3 * ref.max()
        worst = float(np.max(np.abs(dev[big] - ref[big]) / ref[big]))
        # The head's bias receives the plain sum of the logits' gradients, which cancels: every hinge-active (or Wasserstein)
        # real logit gives -1/n, every fake one +1/n, and a pair of the penalty gives +g and -g.  What is left on either side is
        # rounding residue with no direction; such a gradient (norm below 1e-6 of the network's largest) has no cosine, and the
        # device's must be as small.
        norms = {k: float(grads[k][0].double().norm()) for k in keys}
        tiny = 1e-6 * max(norms.values())
        for k in [k for k in keys if norms[k] <= tiny]:
            assert float(snaps[tag][k].double().norm()) <= tiny, (tag, k)
            keys.remove(k)
        assert len(keys) >= len(norms) // 2, (tag, norms)                 # (the attention projections behind gamma = 0 are zero too)
        cos = {k: _cos(snaps[tag][k], grads[k][0]) for k in keys}
        moved = {k: _cos(grads[k][1], grads[k][0]) for k in keys}
        print(f"[cr] {adv} {tag}: checksum worst rel {worst:.2e}, cosine min {min(cos.values()):.6f}, "
              f"oracle without against with the penalty: cosine min {min(moved.values()):.3f}")
        assert worst < 1e-2, (tag, worst)
        assert min(cos.values()) >= 0.9999, (tag, cos)
        assert min(moved.values()) < 0.99, (tag, moved)


# ------------------------------------------------------------------ 4. nothing reaches the generator in a D iteration
def test_the_generator_gets_no_gradient_in_a_d_iteration():
    B, d_iters = 2, 2
    _seed(29)
    tr = _trainer(B, kw=dict(d_cr=10.0), d_aug_p=1.0, d_iters=d_iters)
    at = []
    _at_adam(tr, lambda tag: at.append((tag, float(tr.g_optimizer.grad.abs().max()))))
    tr.train_step(*_clips(B, 1)[0])
    torch.cuda.synchronize()
    assert [tag for tag, _ in at] == ["Ds", "Dt"] * d_iters and all(v == 0.0 for _, v in at), at
    assert float(tr.g_optimizer.grad.abs().max()) > 0.0                   # ... and the generator step's own gradient is there


# ------------------------------------------------------------------ 5. identity transform
def test_identity_transform_gives_no_gap():
    """d_aug_p = 0: every pair holds the same clip twice.  Each site's mean squared gap is at most the project's loss tolerance
    squared, (2e-3 max|logit| + 2e-4)^2, and the step's losses agree with the run without the feature to that tolerance."""
    B, runs = 2, []
    clips = _clips(B, 1)[0]
    for kw in (None, dict(d_cr=10.0)):
        _seed(31)
        tr = _trainer(B, kw=kw, d_aug_p=0.0)
        seen = _watch(tr)
        losses = [float(v.detach()) for v in tr.train_step(*clips)]
        runs.append((losses, seen, tr.cr_report()))
    (plain, _, none), (got, seen, rep) = runs
    assert none is None
    np.testing.assert_allclose(got, plain, rtol=2e-3, atol=2e-4)
    for site, (tag, j) in zip(("Ds_real", "Ds_fake", "Dt_real", "Dt_fake"), (("Ds", 0), ("Ds", 1), ("Dt", 0), ("Dt", 1))):
        top = float(seen[tag][j][2].abs().max())
        print(f"[cr] identity {site}: mean squared gap {rep[site]['mean_sq_gap']:.3e}, max |gap| {rep[site]['max_abs_gap']:.3e}, "
              f"max |logit| {top:.3e}, non-zero {rep[site]['nonzero']} of {rep[site]['n']}")
        assert rep[site]["mean_sq_gap"] <= (2e-3 * top + 2e-4) ** 2, site


# ------------------------------------------------------------------ 6. frame-conditional
def test_frame_conditional_clean_view_holds_the_raw_context():
    B, n_cond = 2, 4
    F = T + n_cond
    (clips, labels), draws = _clips(B, 1, frames=F)[0], _draws(B, **_tables(B, 71))
    seen = []
    for kw in (None, dict(d_cr=10.0)):
        _seed(13)
        tr = _trainer(B, kw=kw, d_aug_p=1.0, n_cond=n_cond)
        seen.append(_watch(tr))
        tr.train_step(clips, labels, draws)
        torch.cuda.synchronize()
    plain, cr = seen
    real5 = clips.permute(0, 2, 1, 3, 4).contiguous().to(DEV)           # [B, F, 3, H, W]
    fake5 = cr["G"][0]
    assert tuple(fake5.shape) == (B, T, 3, S, S)
    x, _, _ = cr["Dt"][1]
    assert tuple(x.shape) == (2 * B, 3, F, S // 2, S // 2)
    assert torch.equal(_bits(x[:B]), _bits(plain["Dt"][1][0]))            # the transformed half: today's [T(context) | T(fake)]
    whole = torch.cat([real5[:, :n_cond], fake5], 1).double()             # [raw context | generated]
    want = whole.view(B, F, 3, S // 2, 2, S // 2, 2).mean((4, 6)).permute(0, 2, 1, 3, 4)
    # the 2 x 2 average in fp32: three additions and the factor, on values of magnitude <= 1
    assert float((x[B:].double() - want).abs().max()) <= 4 * E32
    assert float((x[:B, :, :n_cond] - x[B:, :, :n_cond]).abs().max()) > 0.05       # the other half's context IS transformed
    # D_s is not shown the context: k target frames, clean ones from the same ids
    from dvd_gan_amd.helpers import sample_k_frames
    ids_real, ids_fake = _ids(draws)
    xs, _, _ = cr["Ds"][0]
    assert tuple(xs.shape) == (2 * B, K, 3, S, S)
    assert torch.equal(_bits(xs[B:]), _bits(sample_k_frames(real5, F, K, ids_real + n_cond)))
    assert torch.equal(_bits(cr["Ds"][1][0][B:]), _bits(sample_k_frames(fake5, T, K, ids_fake)))
    x, _, _ = cr["Dt"][0]
    assert torch.equal(_bits(x[:B]), _bits(plain["Dt"][0][0])) and tuple(x.shape) == (2 * B, 3, F, S // 2, S // 2)


# ------------------------------------------------------------------ 7. resume
def test_resume_continues_bitwise(tmp_path):
    B = 2
    clips = _clips(B, 4)
    kw = dict(d_cr=10.0, d_cr_fake=5.0)
    _seed(3)
    a = _trainer(B, tmp_path / "a", kw=kw, d_aug_p=0.7)
    la = [[_bits(v) for v in a.train_step(*c)] for c in clips]
    torch.cuda.synchronize()

    _seed(3)
    b = _trainer(B, tmp_path / "b", kw=kw, d_aug_p=0.7)
    for c in clips[:2]:
        b.train_step(*c)
    b.save_state(2, wait=True)
    b.close_state()
    del b
    path = os.path.join(str(tmp_path / "b"), "2_state.pt")
    _seed(1234); torch.rand(7); random.random(); np.random.rand()
    fresh = _trainer(B, tmp_path / "b", kw=kw, d_aug_p=0.7)
    assert fresh.load_state(path) == []
    lf = [[_bits(v) for v in fresh.train_step(*c)] for c in clips[2:]]
    torch.cuda.synchronize()
    for step in range(2):
        for x, y in zip(la[2 + step], lf[step]):
            assert torch.equal(x, y), step
    for (tag, _), wa, wf in zip(a._optimizers(), _flats(a), _flats(fresh)):
        assert torch.equal(wa, wf), tag
    from dvd_gan_amd import checkpoint as C
    host = C.load_file(path)["host"]                                     # no new state: the file is what it was
    assert sorted(host["aug"]) == ["adjustments", "generator", "p", "steps"] and not [k for k in host if "cr" in str(k).split("_")]


# ------------------------------------------------------------------ 8. the report
def test_report():
    from dvd_gan_amd import lib as L
    B = 2
    _seed(37)
    tr = _trainer(B, kw=dict(d_cr=10.0, d_cr_fake=5.0), d_aug_p=1.0)
    assert tuple(tr._cr_stats.shape) == (4, L.CR_NSTAT) and tr._cr_stats.is_cuda
    tr.train_step(*_clips(B, 1)[0])
    rep = tr.cr_report()
    assert list(rep) == ["Ds_real", "Ds_fake", "Dt_real", "Dt_fake"]
    for site, row in rep.items():
        assert list(row) == ["penalty", "mean_sq_gap", "max_abs_gap", "nonzero", "n"], site
        n = B * K if site.startswith("Ds") else B * T // 4
        w = 10.0 if site.endswith("real") else 5.0
        assert row["n"] == n and row["nonzero"] == n and row["mean_sq_gap"] > 0.0, (site, row)
        assert row["max_abs_gap"] ** 2 >= row["mean_sq_gap"] * (1 - 4 * E32) and row["max_abs_gap"] ** 2 <= n * row["mean_sq_gap"] * (1 + 4 * E32)
        # the penalty and weight * the reported mean are each ONE fp32 rounding of the same fp64 sum: two roundings apart
        assert abs(row["penalty"] - w * row["mean_sq_gap"]) <= 2 * E32 * row["penalty"] * (1 + E32), (site, row)
