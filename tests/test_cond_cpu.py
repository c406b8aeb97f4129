"""CPU checks of the frame-conditional video-prediction variant (BASELINE configs[4]): the conditional generator's module tree and
state_dict, the configuration and argument checks of Generator / Trainer, and the library entry point dvd_vid_downsample_cat
(declared, exported, compiled without scratch).  The arithmetic is checked on the GPU (tests/test_gpu_cond.py)."""
import argparse
import glob
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gen(n_cond=0, ch=2, ld=4, T=8):
    from dvd_gan_amd.gen_net import Generator
    torch.manual_seed(0)
    return Generator(16, ld, 3, ch, T, n_cond=n_cond)


def _cfg(n_cond, T=8, ch=2):
    return argparse.Namespace(adv_loss="hinge", z_dim=16, g_chn=ch, ds_chn=ch, dt_chn=ch, n_frames=T, lr_schr="const",
                              total_epoch=1, d_iters=1, batch_size=2, g_lr=5e-5, d_lr=5e-5, beta1=0.0, beta2=0.9,
                              n_class=3, k_sample=4, n_cond=n_cond)


def test_unconditional_generator_keeps_its_keys_and_parameter_order():
    from dvd_gan_amd.gen_net import Generator
    torch.manual_seed(0)
    a = Generator(16, 4, 3, 2, 8)
    torch.manual_seed(0)
    b = Generator(16, 4, 3, 2, 8, n_cond=0)
    assert list(a.state_dict()) == list(b.state_dict())
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    assert not hasattr(b, "cond_encoder")
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), n                 # same initialisation draws: nothing new is drawn when n_cond == 0


def expected_encoder_shapes(K, ch):
    c2, c4, c8 = 2 * ch, 4 * ch, 8 * ch

    def sn(pfx, cin, cout, k):
        return {pfx + "module.bias": (cout,), pfx + "module.weight_u": (cout,), pfx + "module.weight_v": (cin * k * k,),
                pfx + "module.weight_bar": (cout, cin, k, k)}
    want = sn("cond_encoder.stem.", 3 * K, c2, 3)
    for i, (ci, co) in enumerate(((c2, c4), (c4, c8), (c8, c8), (c8, c8))):
        p = f"cond_encoder.blocks.{i}."
        want.update(sn(p + "conv0.", ci, co, 3))
        want.update(sn(p + "conv1.", co, co, 3))
        want.update(sn(p + "conv_sc.", ci, co, 1))
    for s in range(4):
        cin = c8 if s < 3 else c4
        hs = (c8, 2 * c8, c8) if s < 3 else (c4, 2 * c4, c4)
        for l, h in enumerate(hs):
            want.update(sn(f"cond_encoder.heads.{s}.{l}.", cin, h, 3))
    return want


@pytest.mark.parametrize("K,ch", [(1, 2), (4, 2), (4, 8)])
def test_conditional_generator_adds_exactly_the_encoder_keys(K, ch):
    base = _gen(0, ch)
    g = _gen(K, ch)
    sd, sd0 = g.state_dict(), base.state_dict()
    assert list(sd)[:len(sd0)] == list(sd0)          # every existing key first, in the same order
    extra = {k: tuple(v.shape) for k, v in sd.items() if k not in sd0}
    assert extra == expected_encoder_shapes(K, ch)
    names = [n for n, _ in g.named_parameters()]
    assert names[:len(list(base.parameters()))] == [n for n, _ in base.named_parameters()]
    assert all(n.startswith("cond_encoder.") for n in names[len(list(base.parameters())):])
    for n, p in g.named_parameters():
        assert p.requires_grad == (not n.endswith(("weight_u", "weight_v"))), n
    from dvd_gan_amd.sn_layers import SpectralNormConv
    # the encoder's SN convs are modules of the generator: prefetch_spectral_norm(G) prepares them in the same batched launch
    assert sum(isinstance(m, SpectralNormConv) for m in g.cond_encoder.modules()) == 1 + 4 * 3 + 12


def test_generator_argument_checks():
    K, B = 2, 2
    g = _gen(K)
    z, c = torch.randn(B, 16), torch.zeros(B, dtype=torch.long)
    cond = torch.zeros(B, K, 3, 64, 64)
    hidden = [[None] * 3 for _ in range(4)]
    with pytest.raises(ValueError, match="not `hidden`"):
        g(z, c, hidden=hidden, cond=cond)
    with pytest.raises(ValueError, match="needs the context frames"):
        g(z, c)
    with pytest.raises(ValueError, match="cond must be"):
        g(z, c, cond=torch.zeros(B, K + 1, 3, 64, 64))           # wrong K
    with pytest.raises(ValueError, match="cond must be"):
        g(z, c, cond=torch.zeros(B, K, 3, 32, 32))               # wrong frame size
    with pytest.raises(ValueError, match="cond must be"):
        g(z, c, cond=torch.zeros(B + 1, K, 3, 64, 64))           # wrong batch
    with pytest.raises(ValueError, match="n_cond > 0"):
        _gen(0)(z, c, cond=cond)
    with pytest.raises(ValueError):
        _gen(-1)


@pytest.mark.parametrize("K,T", [(1, 8), (4, 6), (2, 12), (3, 12)])
def test_trainer_rejects_context_lengths_d_t_cannot_pool(K, T):
    from dvd_gan_amd.train_step import Trainer
    with pytest.raises(ValueError, match="multiple of 4"):
        Trainer([], _cfg(K, T), device=torch.device("cpu"), compute_dtype=torch.float32)


def test_trainer_argument_checks():
    from dvd_gan_amd.train_step import Trainer
    tr = Trainer([], _cfg(4, 8), device=torch.device("cpu"), compute_dtype=torch.float32)
    assert tr.n_cond == 4 and hasattr(tr.G, "cond_encoder")
    assert not tr.G.dp_hooks
    real, labels = torch.zeros(2, 3, 12, 64, 64), torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError, match="not from `hidden`"):
        tr.train_step(real, labels, hidden=[[None] * 3 for _ in range(4)])
    with pytest.raises(ValueError, match="n_cond \\+ n_frames = 12"):
        tr.train_step(torch.zeros(2, 3, 8, 64, 64), labels)
    with pytest.raises(RuntimeError, match="predict"):
        tr.sample(torch.zeros(2, 16), labels)
    assert tr.G.training
    plain = Trainer([], _cfg(0, 8), device=torch.device("cpu"), compute_dtype=torch.float32)
    assert plain.n_cond == 0 and not hasattr(plain.G, "cond_encoder")
    with pytest.raises(RuntimeError, match="n_cond > 0"):
        plain.predict(torch.zeros(2, 4, 3, 64, 64), labels)


def test_vid_downsample_cat_is_declared_and_exported():
    import ctypes
    from dvd_gan_amd import lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvdgan_hip.h")).read(), flags=re.S)
    assert re.search(r"int dvd_vid_downsample_cat\(const float\* a, int Ta, float\* b, int Tb, float\* dst, int B, int C, "
                     r"int H, int W, int backward,\s+void\* stream\);", src)
    lib = L.lib()
    assert hasattr(lib, "dvd_vid_downsample_cat")
    assert lib.dvd_abi_version() == 13 == L.ABI_VERSION
    f = lib.dvd_vid_downsample_cat
    p = ctypes.c_void_p(16)                        # never dereferenced: every call below is refused before a launch
    assert f(None, 4, p, 12, p, 2, 3, 64, 64, 0, None) == -1        # forward needs the context
    assert f(p, 4, None, 12, p, 2, 3, 64, 64, 1, None) == -1
    assert f(p, 0, p, 12, p, 2, 3, 64, 64, 0, None) == -1
    assert f(p, 4, p, 0, p, 2, 3, 64, 64, 0, None) == -1
    assert f(p, 4, p, 12, p, 2, 3, 63, 64, 0, None) == -2
    assert f(p, 4, p, 12, p, 2, 3, 64, 30 + 1, 1, None) == -2


def test_vid_downsample_cat_kernel_uses_no_scratch():
    """hipcc's resource report of the new kernel (csrc/build.sh keeps it as build/<file>.res), as tests/test_abi_cpu.py reads it."""
    files = sorted(glob.glob(os.path.join(ROOT, "dvd_gan_amd", "csrc", "build", "pointwise.res")))
    if not files:
        pytest.skip("no build/pointwise.res: the library was not built by csrc/build.sh in this tree")
    name, rec, found = None, {}, None
    for line in open(files[0]):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            if name and "vid_down_cat_kernel" in name:
                found = rec
            name, rec = m.group(1), {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and name:
            rec[m.group(1).strip()] = int(m.group(2))
    if name and "vid_down_cat_kernel" in name:
        found = rec
    assert found, "vid_down_cat_kernel missing from the resource report"
    assert found["ScratchSize"] == 0 and found["VGPRs Spill"] == 0 and found["SGPRs Spill"] == 0, found
