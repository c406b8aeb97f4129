"""The Trainer's latent consistency regularization (Trainer(z_cr=, z_cr_gen=, z_cr_sigma=)): off is the step as it was; on, the
generator runs once per D iteration on [z | z + dz], every fake call of the discriminators takes the views of both halves, the
penalty's gradient reaches the discriminators as the CPU oracle computes it, the generator's own term sends the restatement's
gradient into both halves of its output, nothing reaches the generator in a D iteration, sigma = 0 is the identity, the
frame-conditional context is repeated, d_cr adds a third group, a resumed run continues bit-equal, and zcr_report() reads the
statistics.  Exact (fp32) mode at tests/test_gpu_cr_trainer.py's widths."""
import argparse
import os
import random

import numpy as np
import pytest
import torch

import zcr_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CH, T, K, NCLS, ZD = 2, 8, 4, 3, 16
S = 64
AUG = "color,translation,cutout"
E32 = 2.0 ** -24
ON = dict(z_cr=5.0, z_cr_gen=0.5)
# The gradient tests' weight and perturbation.  At the reference's initialisation the discriminators' logits move by a few 1e-3
# between G(z) and G(z + dz) for dz of unit scale: on the CPU oracle alone (seed 23, these widths, clean views) z_cr = 5 with unit
# dz gives penalties of 6e-6 (D_s) and 5e-7 (D_t) and a gradient whose cosine against the one without the penalty is 0.9999996 --
# nothing to compare.  The generator's tanh output saturates (mean squared distance 0.012, 0.27, 0.42 at scales 1, 8, 64), so the
# scale is raised to 8 and the rest comes from the weight, in which the penalty is linear: the oracle's penalties on the
# transformed views are 3.6e-6 (D_s) and 3.9e-7 (D_t) per unit of weight, hence 1e4 for 3.6e-2 and 3.9e-3 against the 1e-3 asked.
BIG_W, BIG_DZ = 10000.0, 8.0


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
    """Rows that transform EVERY clip (p = 1): brightness / saturation / contrast, a shift and a cutout."""
    from dvd_gan_amd.augment import draw_params
    gen = torch.Generator().manual_seed(seed)
    return {"aug_real": draw_params(B, S, S, AUG, 1.0, gen), "aug_fake": draw_params(B, S, S, AUG, 1.0, gen)}


def _draws(B, seed=3, dz=1.0, **tables):
    g = torch.Generator().manual_seed(seed)
    d = {"perm_real": torch.randperm(T, generator=g), "z": torch.randn(B, ZD, generator=g),
         "z_class": torch.randint(0, NCLS, (B,), generator=g), "perm_fake": torch.randperm(T, generator=g)}
    d["z_delta"] = dz * torch.randn(B, ZD, generator=g)
    d.update(tables)
    return d


def _watch(tr, grads=None):
    """Record (input, labels, logits) of every call of the two discriminators and (z, labels, cond, output) of every call of the
    generator, in order; `grads` (a list) receives the gradient arriving at each generator output."""
    seen = {"Ds": [], "Dt": [], "G": []}
    for tag, net in (("Ds", tr.D_s), ("Dt", tr.D_t)):
        def forward(*a, _orig=net.forward, _tag=tag, **kw):
            out = _orig(*a, **kw)
            seen[_tag].append((a[0].detach().clone(), a[1].detach().clone(), out.detach().clone()))
            return out
        net.forward = forward

    def g_forward(x, class_id, hidden=None, cond=None, _orig=tr.G.forward):
        out = _orig(x, class_id, hidden, cond=cond)
        seen["G"].append((x.detach().clone(), class_id.detach().clone(), None if cond is None else cond.detach().clone(),
                          out.detach().clone()))
        if grads is not None and out.requires_grad:
            out.register_hook(lambda g: grads.append(g.detach().clone()))
        return out
    tr.G.forward = g_forward
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


def _view(clips, table):
    """What the step shows the discriminators of generated clips [B, T, 3, H, W] under the table rows `table` (None: as they are)."""
    from dvd_gan_amd.train_step import Trainer
    clips = clips.contiguous()
    return clips if table is None else Trainer._d_view(clips, None, torch.as_tensor(table, dtype=torch.float32).contiguous().to(DEV))


# ------------------------------------------------------------------ 1. off is the parent
def test_off_is_the_step_without_the_keywords():
    B, runs = 2, []
    for kw in (None, dict(z_cr=0.0), dict(z_cr=0.0, z_cr_gen=0.0, z_cr_sigma=0.5)):
        _seed(5)
        tr = _trainer(B, kw=kw, d_aug_p=0.7)
        losses = [[_bits(v) for v in tr.train_step(*c)] for c in _clips(B, 2)]
        torch.cuda.synchronize()
        assert tr.noise_gen is None                         # a single process draws z from the default generator
        runs.append((losses, _flats(tr), torch.get_rng_state()))
        assert tr._zcr_stats is None and tr._zcr_stats_g is None and tr.zcr_report() is None and tr.z_cr == tr.z_cr_gen == 0.0
    for lb, fb, rb in runs[1:]:
        for step in range(2):
            for a, b in zip(runs[0][0][step], lb[step]):
                assert torch.equal(a, b), step
        for a, b in zip(runs[0][1], fb):
            assert torch.equal(a, b)
        assert torch.equal(runs[0][2], rb)


# ------------------------------------------------------------------ 2. what the networks are given
@pytest.mark.parametrize("d_iters", [1, 2])
def test_what_the_networks_are_given(d_iters):
    from dvd_gan_amd.helpers import sample_k_frames, vid_downsample
    B = 2
    (clips, labels) = _clips(B, 1)[0]
    draws = [_draws(B, seed=3 + i, **_tables(B, 50 + i)) for i in range(d_iters)]
    seen = []
    for kw in (None, ON):
        _seed(7)
        tr = _trainer(B, kw=kw, d_aug_p=1.0, d_iters=d_iters)
        seen.append(_watch(tr))
        tr.train_step(clips, labels, draws if d_iters > 1 else draws[0])
        torch.cuda.synchronize()
    plain, on = seen
    assert [len(on[k]) for k in ("Ds", "Dt", "G")] == [2 * d_iters + 1, 2 * d_iters + 1, d_iters]
    for it in range(d_iters):
        d = draws[it]
        _, ids_fake = _ids(d)
        # the generator: ONE call on 2B rows [z | z + z_delta], labels repeated
        z, cls, cond, out = on["G"][it]
        assert tuple(z.shape) == (2 * B, ZD) and cond is None and tuple(out.shape) == (2 * B, T, 3, S, S)
        assert torch.equal(z[:B].cpu(), d["z"]) and torch.equal(z[B:].cpu(), (d["z"].to(DEV) + d["z_delta"].to(DEV)).cpu())
        assert torch.equal(cls.cpu(), torch.cat([d["z_class"], d["z_class"]]))
        assert tuple(plain["G"][it][0].shape) == (B, ZD)
        # every fake call: [views of the base clips | views of the partners], the same table rows and frame ids
        base, part = _view(out[:B], d["aug_fake"]), _view(out[B:], d["aug_fake"])
        assert not torch.equal(base, out[:B])                                # the rows transform every clip
        want = {"Ds": torch.cat([sample_k_frames(base, T, K, ids_fake), sample_k_frames(part, T, K, ids_fake)]),
                "Dt": torch.cat([vid_downsample(base), vid_downsample(part)])}
        for tag in ("Ds", "Dt"):
            x, lab, logits = on[tag][2 * it + 1]
            x0, lab0, logits0 = plain[tag][2 * it + 1]
            assert x.shape[0] == 2 * B and tuple(x.shape[1:]) == tuple(x0.shape[1:]) and logits.numel() == 2 * logits0.numel(), tag
            assert torch.equal(_bits(x), _bits(want[tag])), (tag, it)
            assert not torch.equal(x[:B], x[B:])
            assert torch.equal(lab.cpu(), torch.cat([d["z_class"], d["z_class"]])) and torch.equal(lab0.cpu(), d["z_class"])
            # the real call is the parent's, to the bit (it does not depend on the generator)
            xr, labr, _ = on[tag][2 * it]
            xr0, labr0, _ = plain[tag][2 * it]
            assert xr.shape == xr0.shape and torch.equal(_bits(xr), _bits(xr0)) and torch.equal(labr, labr0), (tag, it)
    # the generator step: B samples, the views of the base half of the last generator call
    for tag in ("Ds", "Dt"):
        x, lab, _ = on[tag][-1]
        x0, lab0, _ = plain[tag][-1]
        assert x.shape == x0.shape and x.shape[0] == B and torch.equal(lab, lab0)
        assert torch.equal(_bits(x), _bits(want[tag][:B])), tag


# ------------------------------------------------------------------ 3. gradient parity with the oracle
def _cos(a, b):
    """tests/test_gpu_trainer.py's: 1.0 when both gradients are exactly zero (attention behind gamma = 0), 0.0 when one is."""
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    if float(b.norm()) == 0.0:
        return 1.0 if float(a.norm()) == 0.0 else 0.0
    return float((a * b).sum() / (a.norm() * b.norm() + 1e-300))


def _oracle(O, disc, arrays, calls, adv):
    """The oracle discriminator on the recorded inputs, real then fake (u / v advance per call as on the device).  calls: (input,
    labels, real flag, weights) with one weight per partner group behind the first group ->
    (adversarial terms, penalties in call and group order, {parameter: (gradient of their sum, gradient without the penalties)})."""
    sd = O.make_state(arrays)
    outs = [disc(sd, x, cls) for x, cls, _, _ in calls]
    advs, pens = [], []
    for out, (_, _, flag, weights) in zip(outs, calls):
        n = out.numel() // (1 + len(weights))
        advs.append(O.adv_loss(out[:n], flag, adv))
        for i, w in enumerate(weights):
            pens.append(w * ((out[:n] - out[(i + 1) * n:(i + 2) * n]) ** 2).mean())
    prm = O.trainable(sd)
    keys = list(prm)
    plain = torch.autograd.grad(sum(advs), [prm[k] for k in keys], retain_graph=True, allow_unused=True)
    full = torch.autograd.grad(sum(advs) + sum(pens), [prm[k] for k in keys], allow_unused=True)
    grads = {k: (f.detach(), p.detach()) for k, f, p in zip(keys, full, plain) if f is not None}
    return [float(v.detach()) for v in advs], [float(v.detach()) for v in pens], grads


def _check_against_oracle(tag, adv, got_losses, got_pens, snaps, advs, pens, grads):
    """The project's exact-mode tolerances (tests/test_gpu_cr_trainer.py): losses and penalties rtol 2e-3 / atol 2e-4, |grad|
    checksum of every parameter 1e-2 relative (over the parameters whose checksum is above 1e-3 of the largest), named-gradient
    cosine >= 0.9999; and the penalty must matter: the oracle's gradient without it has cosine < 0.99 against the one with it
    for some parameter."""
    print(f"[zcr] {adv} {tag}: losses {got_losses} / {advs}, penalties {got_pens} / {pens}")
    np.testing.assert_allclose(got_losses, advs, rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(got_pens, pens, rtol=2e-3, atol=2e-4)
    assert min(pens) > 1e-3
    keys = list(grads)
    assert keys and set(keys) <= set(snaps)
    ref = np.array([float(grads[k][0].double().abs().sum()) for k in keys])
    dev = np.array([float(snaps[k].double().abs().sum()) for k in keys])
    big = ref > 1e-3 * ref.max()
    worst = float(np.max(np.abs(dev[big] - ref[big]) / ref[big]))
    # (the head's bias receives a sum that cancels to rounding residue: no direction, see tests/test_gpu_cr_trainer.py)
    norms = {k: float(grads[k][0].double().norm()) for k in keys}
    tiny = 1e-6 * max(norms.values())
    for k in [k for k in keys if norms[k] <= tiny]:
        assert float(snaps[k].double().norm()) <= tiny, (tag, k)
        keys.remove(k)
    assert len(keys) >= len(norms) // 2, (tag, norms)
    cos = {k: _cos(snaps[k], grads[k][0]) for k in keys}
    moved = {k: _cos(grads[k][1], grads[k][0]) for k in keys}
    print(f"[zcr] {adv} {tag}: checksum worst rel {worst:.2e}, cosine min {min(cos.values()):.6f}, "
          f"oracle without against with the penalty: cosine min {min(moved.values()):.3f}")
    assert worst < 1e-2, (tag, worst)
    assert min(cos.values()) >= 0.9999, (tag, cos)
    assert min(moved.values()) < 0.99, (tag, moved)


def _gradient_run(adv, kw, seed):
    B = 2
    _seed(seed)
    tr = _trainer(B, kw=kw, adv_loss=adv, d_aug_p=1.0)
    arrays = {tag: {k: v.detach().cpu().clone() for k, v in net.state_dict().items()} for tag, net in (("Ds", tr.D_s), ("Dt", tr.D_t))}
    seen, snaps = _watch(tr), {}
    nets = {"Ds": tr.D_s, "Dt": tr.D_t}
    _at_adam(tr, lambda tag: snaps.setdefault(tag, {k: p.grad.detach().cpu().clone() for k, p in nets[tag].named_parameters()
                                                    if p.grad is not None}))
    (clips, labels), draws = _clips(B, 1)[0], _draws(B, dz=BIG_DZ, **_tables(B, 61))
    got = [float(v.detach()) for v in tr.train_step(clips, labels, draws)]
    return tr, arrays, seen, snaps, got


@pytest.mark.parametrize("adv", ["hinge", "wgan-gp"])
def test_discriminator_gradients_match_the_oracle(adv):
    from oracle import dvdgan_cpu as O
    tr, arrays, seen, snaps, got = _gradient_run(adv, dict(z_cr=BIG_W, z_cr_gen=0.5), 23)
    rep = tr.zcr_report()
    for i, (tag, disc) in enumerate((("Ds", O.spatial_disc), ("Dt", O.temporal_disc))):
        calls = [(x.cpu(), cls.cpu(), flag, w) for (x, cls, _), flag, w in zip(seen[tag][:2], (True, False), ((), (BIG_W,)))]
        assert calls[0][0].shape[0] == 2 and calls[1][0].shape[0] == 4
        advs, pens, grads = _oracle(O, disc, arrays[tag], calls, adv)
        _check_against_oracle(tag, adv, got[2 * i:2 * i + 2], [rep[tag]["penalty"]], snaps[tag], advs, pens, grads)


# ------------------------------------------------------------------ 4. the generator-side gradient in place
def test_generator_term_sends_the_restatement_gradient_into_both_halves():
    B = 2
    (clips, labels), draws = _clips(B, 1)[0], _draws(B, **_tables(B, 67))
    runs = []
    for kw in (dict(z_cr=5.0, z_cr_gen=0.0), dict(z_cr=5.0, z_cr_gen=0.5)):
        _seed(41)
        tr = _trainer(B, kw=kw, d_aug_p=1.0)
        grads = []
        seen = _watch(tr, grads)
        losses = [_bits(v) for v in tr.train_step(clips, labels, draws)]
        torch.cuda.synchronize()
        assert len(grads) == 1 and tuple(grads[0].shape) == (2 * B, T, 3, S, S)
        runs.append((losses, _flats(tr), grads[0].cpu(), seen["G"][0][3].cpu(), tr.zcr_report()))
    (la, fa, ga, outa, repa), (lb, fb, gb, outb, repb) = runs
    # up to the generator step the two runs are the same run: D losses, the D weights after their Adam, the generator's output
    for x, y in zip(la[:4], lb[:4]):
        assert torch.equal(x, y)
    assert torch.equal(fa[1], fb[1]) and torch.equal(fa[2], fb[2]) and torch.equal(_bits(outa), _bits(outb))
    assert not torch.equal(fa[0], fb[0])                                        # ... and the term moves the generator
    # A: nothing reaches the partner half.  B: the partner half is the restatement's db of the recorded output, to the bit
    # (autograd adds it to zeros: a -0 arrives as +0, so values are compared)
    assert float(ga[B:].abs().max()) == 0.0 and float(ga[:B].abs().max()) > 0.0
    both = outb.numpy().reshape(2 * B, -1)
    want_da, want_db = R.grad(both[:B], both[B:], 0.5, 1.0)
    assert np.array_equal(gb[B:].numpy().reshape(B, -1), want_db)
    assert float(np.abs(want_db).max()) > 0.0
    # B's base half is fl32(A's + da), da = -db to the bit: ONE fp32 addition, so base + partner (exact in fp64) misses A's base
    # half by that addition's rounding, at most 2^-24 of ITS result -- asserted on every element.  Relative to A's own element
    # that is 2^-24 (|A| + |db|) / |A|: within 4 * 2^-24 wherever |db| <= 3 |A|, asserted there on the elements above 1e-6 of the
    # largest; where the D path's gradient is far smaller than db (measured: 2.4e-4 relative at |A| = 1e-6 of the largest, |db|
    # up to 1e-5 against a largest |A| of 4e-5) no fp32 sum can do better.
    a_base, b_base, b_part = ga[:B].double(), gb[:B].double(), gb[B:].double()
    err = (b_base + b_part - a_base).abs()
    assert bool((err <= E32 * b_base.abs()).all()), float((err - E32 * b_base.abs()).max())
    top = float(a_base.abs().max())
    mask = (a_base.abs() > 1e-6 * top) & (b_part.abs() <= 3 * a_base.abs())
    rel = (err / a_base.abs())[mask]
    print(f"[zcr] base + partner against the run without the term: worst relative {float(rel.max()):.3e} over {int(mask.sum())} of "
          f"{mask.numel()} elements; |db| max {float(np.abs(want_db).max()):.3e}, |D path| max {top:.3e}")
    assert int(mask.sum()) > 0 and float(rel.max()) <= 4 * E32
    # the reports: A measures the distance without a term, B's term is the restatement's
    ref = R.dist(both[:B], both[B:], 0.5)
    assert repa["G"]["term"] == 0.0 and repa["G"]["mean_sq_dist"] == repb["G"]["mean_sq_dist"] > 0.0
    assert R.ulps(np.float32(repb["G"]["term"]), ref["term"]) <= 2 and repb["G"]["max_abs_diff"] == float(ref["max_abs_diff"])


# ------------------------------------------------------------------ 5. nothing reaches the generator in a D iteration
def test_the_generator_gets_no_gradient_in_a_d_iteration():
    B, d_iters = 2, 2
    _seed(29)
    tr = _trainer(B, kw=ON, d_aug_p=1.0, d_iters=d_iters)
    at = []
    _at_adam(tr, lambda tag: at.append((tag, float(tr.g_optimizer.grad.abs().max()))))
    tr.train_step(*_clips(B, 1)[0])
    torch.cuda.synchronize()
    assert [tag for tag, _ in at] == ["Ds", "Dt"] * d_iters and all(v == 0.0 for _, v in at), at
    assert float(tr.g_optimizer.grad.abs().max()) > 0.0                   # ... and the generator step's own gradient is there


# ------------------------------------------------------------------ 6. identity
def test_sigma_zero_is_the_identity(monkeypatch):
    """z_cr_sigma = 0 with no `draws`: the generator is given every row twice.  A duplicated batch has the same batch-norm
    statistics, and condition row (b T + t) mod 2B of it is row (b T + t) mod B of the plain one, so the base half is the parent's
    output up to rounding: each site's mean squared gap is at most the project's loss tolerance squared, (2e-3 max|logit| +
    2e-4)^2, the generator's mean squared distance at most (2e-3 + 2e-4)^2 (outputs in [-1, 1]), and the six losses agree with
    the parent run on the same draws at rtol 2e-3 / atol 2e-4."""
    import dvd_gan_amd.train_step as TS
    B = 2
    clips = _clips(B, 1)[0]
    drawn = []
    orig = TS.draw_frame_ids
    monkeypatch.setattr(TS, "draw_frame_ids", lambda *a, **kw: drawn.append(orig(*a, **kw)) or drawn[-1])
    _seed(31)
    tr = _trainer(B, kw=dict(z_cr=5.0, z_cr_gen=0.5, z_cr_sigma=0.0), d_aug_p=0.7)
    seen = _watch(tr)
    got = [float(v.detach()) for v in tr.train_step(*clips)]
    rep = tr.zcr_report()
    z, cls, _, out = seen["G"][0]
    assert torch.equal(z[:B], z[B:]) and torch.equal(cls[:B], cls[B:]) and len(drawn) == 2
    # the parent on the draws this run made (its tables come from the private generator, seeded alike)
    _seed(31)
    parent = _trainer(B, d_aug_p=0.7)
    draws = {"perm_real": drawn[0].cpu(), "z": z[:B].cpu(), "z_class": cls[:B].cpu(), "perm_fake": drawn[1].cpu()}
    plain = [float(v.detach()) for v in parent.train_step(*clips, draws)]
    print(f"[zcr] identity: losses {got} / parent {plain}")
    np.testing.assert_allclose(got, plain, rtol=2e-3, atol=2e-4)
    for tag in ("Ds", "Dt"):
        top = float(seen[tag][1][2].abs().max())
        print(f"[zcr] identity {tag}: mean squared gap {rep[tag]['mean_sq_gap']:.3e}, max |gap| {rep[tag]['max_abs_gap']:.3e}, "
              f"max |logit| {top:.3e}, non-zero {rep[tag]['nonzero']} of {rep[tag]['n']}")
        assert rep[tag]["mean_sq_gap"] <= (2e-3 * top + 2e-4) ** 2, tag
    print(f"[zcr] identity G: {rep['G']}")
    assert rep["G"]["mean_sq_dist"] <= (2e-3 + 2e-4) ** 2 and rep["G"]["pairs"] == B
    assert float((out[:B] - out[B:]).abs().max()) == rep["G"]["max_abs_diff"]


# ------------------------------------------------------------------ 7. frame-conditional
def test_frame_conditional_repeats_the_context():
    from dvd_gan_amd.helpers import sample_k_frames, vid_downsample_cat
    B, n_cond = 2, 4
    F = T + n_cond
    (clips, labels), draws = _clips(B, 1, frames=F)[0], _draws(B, **_tables(B, 71))
    _seed(13)
    tr = _trainer(B, kw=ON, d_aug_p=1.0, n_cond=n_cond)
    seen = _watch(tr)
    tr.train_step(clips, labels, draws)
    torch.cuda.synchronize()
    real5 = clips.permute(0, 2, 1, 3, 4).contiguous().to(DEV)           # [B, F, 3, H, W]
    ctx = real5[:, :n_cond].contiguous()
    z, cls, cond, out = seen["G"][0]
    assert tuple(cond.shape) == (2 * B, n_cond, 3, S, S) and torch.equal(cond[:B], ctx) and torch.equal(cond[B:], ctx)
    assert tuple(out.shape) == (2 * B, T, 3, S, S) and tuple(z.shape) == (2 * B, ZD)
    _, ids_fake = _ids(draws)
    base, part, ctx_in = _view(out[:B], draws["aug_fake"]), _view(out[B:], draws["aug_fake"]), _view(ctx, draws["aug_fake"])
    # D_t's fake call: [ctx | base], [ctx | partner], the context views equal
    x, _, _ = seen["Dt"][1]
    assert tuple(x.shape) == (2 * B, 3, F, S // 2, S // 2)
    assert torch.equal(_bits(x[:B]), _bits(vid_downsample_cat(ctx_in, base))) and torch.equal(_bits(x[B:]), _bits(vid_downsample_cat(ctx_in, part)))
    assert torch.equal(x[:B, :, :n_cond], x[B:, :, :n_cond]) and not torch.equal(x[:B, :, n_cond:], x[B:, :, n_cond:])
    # D_s never sees the context: k target frames of both halves
    xs, _, _ = seen["Ds"][1]
    assert tuple(xs.shape) == (2 * B, K, 3, S, S)
    assert torch.equal(_bits(xs), _bits(torch.cat([sample_k_frames(base, T, K, ids_fake), sample_k_frames(part, T, K, ids_fake)])))
    # the real calls and the generator step's calls have B rows
    assert seen["Ds"][0][0].shape[0] == seen["Dt"][0][0].shape[0] == seen["Ds"][2][0].shape[0] == seen["Dt"][2][0].shape[0] == B
    assert torch.equal(_bits(seen["Dt"][2][0]), _bits(x[:B]))


# ------------------------------------------------------------------ 8. with d_cr as well
@pytest.mark.parametrize("adv", ["hinge"])
def test_with_balanced_consistency_the_fake_calls_hold_three_groups(adv):
    from oracle import dvdgan_cpu as O
    from dvd_gan_amd.helpers import sample_k_frames, vid_downsample
    B = 2
    kw = dict(d_cr=10.0, d_cr_fake=5.0, z_cr=BIG_W, z_cr_gen=0.5)
    tr, arrays, seen, snaps, got = _gradient_run(adv, kw, 23)
    rep, cr_rep = tr.zcr_report(), tr.cr_report()
    draws = _draws(B, dz=BIG_DZ, **_tables(B, 61))
    _, ids_fake = _ids(draws)
    out = seen["G"][0][3]
    base, part = _view(out[:B], draws["aug_fake"]), _view(out[B:], draws["aug_fake"])
    # [T(base) | clean base | T(partners)]
    want = {"Ds": torch.cat([sample_k_frames(base, T, K, ids_fake), sample_k_frames(out[:B].contiguous(), T, K, ids_fake),
                             sample_k_frames(part, T, K, ids_fake)]),
            "Dt": torch.cat([vid_downsample(base), vid_downsample(out[:B].contiguous()), vid_downsample(part)])}
    for i, (tag, disc) in enumerate((("Ds", O.spatial_disc), ("Dt", O.temporal_disc))):
        assert seen[tag][0][0].shape[0] == 2 * B and seen[tag][1][0].shape[0] == 3 * B and seen[tag][2][0].shape[0] == B
        assert torch.equal(_bits(seen[tag][1][0]), _bits(want[tag])), tag
        assert torch.equal(seen[tag][1][1].cpu(), torch.cat([draws["z_class"]] * 3))
        calls = [(x.cpu(), cls.cpu(), flag, w)
                 for (x, cls, _), flag, w in zip(seen[tag][:2], (True, False), ((10.0,), (5.0, BIG_W)))]
        advs, pens, grads = _oracle(O, disc, arrays[tag], calls, adv)
        got_pens = [cr_rep[f"{tag}_real"]["penalty"], cr_rep[f"{tag}_fake"]["penalty"], rep[tag]["penalty"]]
        _check_against_oracle(tag, adv, got[2 * i:2 * i + 2], got_pens, snaps[tag], advs, pens, grads)
    # cr_report() is what it is today: four sites, five fields, n per site
    assert list(cr_rep) == ["Ds_real", "Ds_fake", "Dt_real", "Dt_fake"]
    for site, row in cr_rep.items():
        assert list(row) == ["penalty", "mean_sq_gap", "max_abs_gap", "nonzero", "n"]
        assert row["n"] == (B * K if site.startswith("Ds") else B * T // 4) and row["mean_sq_gap"] > 0.0


# ------------------------------------------------------------------ 9. resume
def test_resume_continues_bitwise(tmp_path):
    B = 2
    clips = _clips(B, 4)
    kw = dict(z_cr=5.0, z_cr_gen=0.5, z_cr_sigma=0.25)
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
    # no new state: the file's host keys are those of a run without the feature
    from dvd_gan_amd import checkpoint as C
    host = C.load_file(path)["host"]
    _seed(3)
    plain = _trainer(B, tmp_path / "c", d_aug_p=0.7)
    plain.train_step(*clips[0])
    plain.save_state(1, wait=True)
    plain.close_state()
    host0 = C.load_file(os.path.join(str(tmp_path / "c"), "1_state.pt"))["host"]
    assert sorted(map(str, host)) == sorted(map(str, host0)) and not [k for k in host if "zcr" in str(k) or "z_cr" in str(k)]


# ------------------------------------------------------------------ 10. the report
def test_report():
    from dvd_gan_amd import lib as L
    B = 2
    reps = []
    for _ in range(2):
        _seed(37)
        tr = _trainer(B, kw=dict(z_cr=5.0, z_cr_gen=0.5, z_cr_sigma=0.5), d_aug_p=1.0)
        assert tuple(tr._zcr_stats.shape) == (2, L.CR_NSTAT) and tuple(tr._zcr_stats_g.shape) == (L.ZCR_NSTAT,) and tr._zcr_stats.is_cuda
        assert tr._cr_stats is None                         # the bCR table keeps its shape and its meaning: it is not there
        tr.train_step(*_clips(B, 1)[0])
        reps.append(tr.zcr_report())
    rep = reps[0]
    assert list(rep) == ["Ds", "Dt", "G"]
    for tag in ("Ds", "Dt"):
        row = rep[tag]
        assert list(row) == ["penalty", "mean_sq_gap", "max_abs_gap", "nonzero", "n"], tag
        n = B * K if tag == "Ds" else B * T // 4
        assert row["n"] == n and 0 < row["nonzero"] <= n and row["mean_sq_gap"] > 0.0, (tag, row)
        assert abs(row["penalty"] - 5.0 * row["mean_sq_gap"]) <= 2 * E32 * row["penalty"] * (1 + E32), (tag, row)
    g = rep["G"]
    assert list(g) == ["term", "mean_sq_dist", "min_pair", "max_pair", "max_abs_diff", "pairs"]
    assert g["pairs"] == B and g["mean_sq_dist"] > 0.0 and 0.0 < g["max_abs_diff"] <= 2.0
    # the term and -z_cr_gen * the reported mean are each ONE fp32 rounding of the same fp64 value: two roundings apart
    assert abs(g["term"] + 0.5 * g["mean_sq_dist"]) <= 2 * E32 * abs(g["term"]) * (1 + E32), g
    assert g["min_pair"] <= g["mean_sq_dist"] <= g["max_pair"] and g["max_abs_diff"] ** 2 >= g["max_pair"] * (1 - 4 * E32)
    print(f"[zcr] report {rep}")
    assert reps[0] == reps[1]                               # two identical runs report identical bits
