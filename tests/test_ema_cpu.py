"""CPU checks of the generator weight average (EMA): argument validation of the three C entry points without a GPU, the truncated
normal of the truncation trick, and the host-side switches (no average -> nothing allocated, use_ema without one -> an error)."""
import ctypes
import math

import pytest
import torch


def test_ema_entry_points_validate_arguments_without_a_gpu():
    """DVD_E_ARG (-1) before any launch: null pointers, n = 0, step = 0, a decay outside [0, 1).  The placeholder pointers
    are never dereferenced."""
    from dvd_gan_amd import lib as L
    lib = L.lib()
    p = ctypes.c_void_p(16)
    f = ctypes.c_float
    n = ctypes.c_longlong(8)
    adam = lambda ptrs, n_, step, decay: lib.dvd_adam_ema_step(*ptrs, n_, f(2e-3), f(0.0), f(0.9), f(1e-8), step, f(decay), None)
    for k in range(5):
        ptrs = [p] * 5
        ptrs[k] = None
        assert adam(ptrs, n, 1, 0.9) == -1, k
    assert adam([p] * 5, ctypes.c_longlong(0), 1, 0.9) == -1
    assert adam([p] * 5, ctypes.c_longlong(-4), 1, 0.9) == -1
    assert adam([p] * 5, n, 0, 0.9) == -1
    for bad in (1.0, 1.5, -0.1, float("nan")):
        assert adam([p] * 5, n, 1, bad) == -1, bad
        assert lib.dvd_ema_step(p, p, n, f(bad), None) == -1, bad
    assert lib.dvd_ema_step(None, p, n, f(0.5), None) == -1
    assert lib.dvd_ema_step(p, None, n, f(0.5), None) == -1
    assert lib.dvd_ema_step(p, p, ctypes.c_longlong(0), f(0.5), None) == -1
    assert lib.dvd_swap_f32(None, p, n, None) == -1
    assert lib.dvd_swap_f32(p, None, n, None) == -1
    assert lib.dvd_swap_f32(p, p, ctypes.c_longlong(0), None) == -1
    assert lib.dvd_abi_version() == 13          # additions only: no signature changed


@pytest.mark.parametrize("tau", [0.04, 0.5, 1.0, 2.0])
def test_truncated_z_bound_seed_and_second_moment(tau):
    """helpers.truncated_z: |z| <= tau, equal output for equal generator seeds, and the second moment of 4096 x 120 draws within
    5 standard errors of the truncated normal's 1 - 2 tau phi(tau) / (2 Phi(tau) - 1)."""
    from dvd_gan_amd.helpers import truncated_z
    B, zd = 4096, 120
    z = truncated_z(B, zd, tau, generator=torch.Generator().manual_seed(0))
    assert z.dtype == torch.float32 and tuple(z.shape) == (B, zd)
    assert float(z.double().abs().max()) <= tau
    assert torch.equal(z, truncated_z(B, zd, tau, generator=torch.Generator().manual_seed(0)))
    assert not torch.equal(z, truncated_z(B, zd, tau, generator=torch.Generator().manual_seed(1)))
    phi = math.exp(-0.5 * tau * tau) / math.sqrt(2.0 * math.pi)
    mass = math.erf(tau / math.sqrt(2.0))                                  # 2 Phi(tau) - 1
    m2 = 1.0 - 2.0 * tau * phi / mass
    # fourth moment of the truncated normal (integration by parts): 3 m2 - 2 tau^3 phi / mass
    m4 = 3.0 * m2 - 2.0 * tau ** 3 * phi / mass
    se = math.sqrt((m4 - m2 * m2) / (B * zd))
    got = float((z.double() ** 2).mean())
    print(f"tau={tau}: second moment {got:.6f}, want {m2:.6f}, {abs(got - m2) / se:.2f} standard errors")
    assert abs(got - m2) <= 5.0 * se, (got, m2, se)
    assert abs(float(z.double().mean())) <= 5.0 * math.sqrt(m2 / (B * zd))


def test_truncated_z_uses_only_the_given_generator():
    from dvd_gan_amd.helpers import truncated_z
    state = torch.get_rng_state()
    truncated_z(4, 8, 0.5, generator=torch.Generator().manual_seed(3))
    assert torch.equal(state, torch.get_rng_state())
    with pytest.raises(ValueError):
        truncated_z(4, 8, 0.0)


def test_flat_adam_without_average_allocates_nothing():
    from dvd_gan_amd.optim import FlatAdam
    params = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7))]
    opt = FlatAdam(params, 1e-3)
    assert opt.ema is None and opt.ema_decay == 0.0
    with pytest.raises(RuntimeError):
        opt.load_ema(torch.zeros(22))
    on = FlatAdam([torch.nn.Parameter(torch.randn(4))], 1e-3, ema_decay=0.9, ema_start=2)
    assert on.ema is None                       # allocated at the first step, from the weights that step starts from
    on.load_ema(torch.arange(4.0))
    assert torch.equal(on.ema, torch.arange(4.0)) and on.ema.data_ptr() != on.flat.data_ptr()
    with pytest.raises(ValueError):
        on.load_ema(torch.zeros(5))
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError):
            FlatAdam([torch.nn.Parameter(torch.randn(4))], 1e-3, ema_decay=bad)


def _cpu_trainer(ema_decay):
    """A Trainer that never ran __init__ (no GPU here), as tests/test_checkpoint_cpu.py builds one."""
    from dvd_gan_amd.gen_net import Generator
    from dvd_gan_amd.optim import FlatAdam
    from dvd_gan_amd.train_step import Trainer
    tr = Trainer.__new__(Trainer)
    tr.G = Generator(16, 4, 3, 2, 8)
    tr.n_cond, tr.z_dim, tr.noise_gen, tr.device = 0, 16, None, torch.device("cpu")
    tr.g_optimizer = FlatAdam(tr.G.parameters(), 1e-3, ema_decay=ema_decay)
    return tr


def test_use_ema_without_a_configured_average_raises():
    tr = _cpu_trainer(0.0)
    with pytest.raises(RuntimeError, match="ema_decay"):
        tr.sample(torch.zeros(2, 16), torch.zeros(2, dtype=torch.long), use_ema=True)
    with pytest.raises(RuntimeError, match="ema_decay"):
        with tr.ema_weights():
            pass
    tr.n_cond = 4
    with pytest.raises(RuntimeError, match="ema_decay"):
        tr.predict(torch.zeros(2, 4, 3, 64, 64), torch.zeros(2, dtype=torch.long), torch.zeros(2, 16), use_ema=True)


def test_truncation_with_a_callers_z_raises():
    tr = _cpu_trainer(0.9)
    with pytest.raises(ValueError, match="truncation"):
        tr.sample(torch.zeros(2, 16), torch.zeros(2, dtype=torch.long), truncation=0.5)
    tr.n_cond = 4
    with pytest.raises(ValueError, match="truncation"):
        tr.predict(torch.zeros(2, 4, 3, 64, 64), torch.zeros(2, dtype=torch.long), torch.zeros(2, 16), truncation=0.5)


def test_checkpoint_of_the_average_round_trips_on_the_host(tmp_path):
    """save_models / load_pretrained_model on a Trainer that never ran __init__: before the first step the average is the
    weights themselves, so `{step}_G_ema.pth` carries G's own entries under G's keys; loading it fills `ema`."""
    import os
    from dvd_gan_amd.disc_nets import SpatialDiscriminator, TemporalDiscriminator
    tr = _cpu_trainer(0.9)
    tr.D_s, tr.D_t = SpatialDiscriminator(2, 3), TemporalDiscriminator(2, 3)
    tr.model_save_path, tr.pretrained_model = str(tmp_path), 5
    tr.save_models(5)
    live = torch.load(os.path.join(str(tmp_path), "5_G.pth"))
    avg = torch.load(os.path.join(str(tmp_path), "5_G_ema.pth"))
    assert list(avg) == list(live)
    assert all(torch.equal(avg[k], live[k]) for k in live)
    assert tr.g_optimizer.ema is None
    tr.load_pretrained_model()
    assert torch.equal(tr.g_optimizer.ema, tr.g_optimizer.flat)
    off = _cpu_trainer(0.0)                      # no average: three files, as before
    off.D_s, off.D_t = tr.D_s, tr.D_t
    off.model_save_path = os.path.join(str(tmp_path), "off")
    off.save_models(5)
    assert sorted(os.listdir(off.model_save_path)) == ["5_Ds.pth", "5_Dt.pth", "5_G.pth"]


def test_ema_weights_block_does_not_nest():
    """A second block inside the first would exchange the live weights back in: it raises, and the outer block still closes."""
    tr = _cpu_trainer(0.9)
    with tr.ema_weights():
        with pytest.raises(RuntimeError, match="does not nest"):
            with tr.ema_weights():
                pass
    with tr.ema_weights():          # usable again afterwards
        pass
