"""CPU checks of the prediction metrics: the two C entry points exist and refuse bad calls before any launch (placeholder
pointers, never dereferenced), metrics.psnr, and the best-of-N aggregation of Trainer.evaluate_prediction on a hand-made table."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from dvd_gan_amd import lib as L
    lib = L.lib()
    lib.dvd_frame_metrics_ws_bytes.restype = C.c_longlong
    return lib


def _call(lib, pred=1, target=1, mse=1, ssim=1, B=2, T=3, Cc=3, H=64, W=64, flags=0):
    p = lambda v: C.c_void_p(v) if v else None
    ll = C.c_longlong
    return lib.dvd_frame_metrics(p(pred), ll(T * Cc * H * W), ll(Cc * H * W), ll(H * W),
                                 p(target), ll(T * Cc * H * W), ll(Cc * H * W), ll(H * W),
                                 ll(B), T, Cc, H, W, flags, p(mse), p(ssim), None, None)


def test_header_and_library_agree_on_the_metrics_entry_points():
    lib = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvdgan_hip.h")).read(), flags=re.S)
    for name in ("dvd_frame_metrics_ws_bytes", "dvd_frame_metrics"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
    from dvd_gan_amd import lib as L
    assert lib.dvd_abi_version() == L.ABI_VERSION == 13          # additions only
    assert set(L.STRUCT_MIRRORS) == {0, 1, 2, 3, 4, 5, 6}        # plain arguments: no new descriptor
    assert lib.dvd_frame_metrics_ws_bytes(C.c_longlong(64), 16, 3, 64, 64) >= 0
    m = re.search(r"#define DVD_METRICS_SIGNED (\d+)\s+#define DVD_METRICS_QUANTIZE (\d+)", src)
    from dvd_gan_amd import kern as K
    assert (int(m.group(1)), int(m.group(2))) == (K.METRICS_SIGNED, K.METRICS_QUANTIZE) == (1, 2)


def test_refusals_happen_before_any_launch():
    lib = _lib()
    for missing in ("pred", "target", "mse", "ssim"):
        assert _call(lib, **{missing: 0}) == -1, missing
    for kw in (dict(H=10), dict(W=10), dict(H=257), dict(W=257), dict(H=0), dict(W=-3),
               dict(Cc=0), dict(T=0), dict(B=0), dict(B=-1), dict(flags=4), dict(flags=-1), dict(flags=7)):
        assert _call(lib, **kw) == -2, kw
    # refused shapes win over nothing else: a null pointer is reported first
    assert _call(lib, pred=0, H=5) == -1


def test_psnr():
    from dvd_gan_amd import metrics as M
    got = M.psnr(np.array([0.0, 1.0, 1e-4]))
    assert got.dtype == np.float64
    assert got[0] == math.inf and got[1] == 0.0 and not np.signbit(got[1]) and abs(got[2] - 40.0) < 1e-12
    t = M.psnr(torch.tensor([[1e-2, 0.25]], dtype=torch.float32))
    assert t.shape == (1, 2) and abs(t[0, 0] - 20.0) < 1e-5 and abs(t[0, 1] - 10 * math.log10(4.0)) < 1e-12
    assert float(M.psnr(0.1)) == pytest.approx(10.0)


def test_best_of_n_is_chosen_per_metric():
    """2 clips x 3 samples x horizon 2.  Clip 0: sample 1 has the best PSNR (lowest mse), sample 2 the best SSIM.  Clip 1: sample 0
    is best at both -- though sample 2 has the single best frame of either metric, its mean over the horizon is lower."""
    from dvd_gan_amd import metrics as M
    mse = np.array([[[1e-2, 1e-2], [1e-4, 1e-2], [1e-1, 1e-1]],
                    [[1e-3, 1e-3], [1e-2, 1e-1], [1e-5, 1.0]]])
    ssim = np.array([[[0.5, 0.5], [0.6, 0.5], [0.9, 0.7]],
                     [[0.8, 0.8], [0.1, 0.2], [0.99, 0.0]]])
    out = M.aggregate_prediction(mse, ssim)
    p = -10 * np.log10(mse)
    np.testing.assert_allclose(out["psnr"], p.mean(axis=(0, 1)), rtol=1e-14)
    np.testing.assert_allclose(out["ssim"], ssim.mean(axis=(0, 1)), rtol=1e-14)
    np.testing.assert_allclose(out["psnr_best"], (p[0, 1] + p[1, 0]) / 2, rtol=1e-14)       # [ (40 + 30) / 2, (20 + 30) / 2 ]
    np.testing.assert_allclose(out["psnr_best"], [35.0, 25.0], rtol=1e-12)
    np.testing.assert_allclose(out["ssim_best"], (ssim[0, 2] + ssim[1, 0]) / 2, rtol=1e-14)
    np.testing.assert_allclose(out["ssim_best"], [0.85, 0.75], rtol=1e-12)
    # the two metrics picked different samples of clip 0: neither curve is the other's selection
    assert not np.allclose(out["ssim_best"], (ssim[0, 1] + ssim[1, 0]) / 2)
    assert not np.allclose(out["psnr_best"], (p[0, 2] + p[1, 0]) / 2)
    assert out["table"]["mse"].shape == out["table"]["ssim"].shape == (2, 3, 2)
    np.testing.assert_array_equal(out["table"]["mse"], mse)
    for k in ("psnr", "ssim", "psnr_best", "ssim_best"):
        assert out[k].shape == (2,) and out[k].dtype == np.float64
    # an exactly predicted frame: +inf, and it wins its clip
    mse0 = mse.copy()
    mse0[0, 0, 1] = 0.0
    out0 = M.aggregate_prediction(mse0, ssim)
    assert out0["psnr"][1] == math.inf and out0["psnr_best"][1] == math.inf and math.isfinite(out0["psnr"][0])
    np.testing.assert_allclose(out0["psnr_best"][0], (20.0 + 30.0) / 2, rtol=1e-12)
    with pytest.raises(ValueError):
        M.aggregate_prediction(mse[0], ssim[0])


def test_frame_metrics_rejects_bad_operands_on_the_host():
    from dvd_gan_amd import metrics as M
    a = torch.zeros(2, 3, 3, 16, 16)
    with pytest.raises(ValueError, match=r"\[\.\.\., T, C, H, W\]"):
        M.frame_metrics(a, torch.zeros(2, 3, 3, 16, 17))
    with pytest.raises(ValueError, match="fp32"):
        M.frame_metrics(a.double(), a.double())
    with pytest.raises(ValueError, match="smaller than"):
        M.frame_metrics(a[..., :10, :], a[..., :10, :])
    with pytest.raises(ValueError, match="planes must be contiguous"):
        M.frame_metrics(a[..., ::1, :12], a[..., ::1, :12])     # a column crop: rows no longer follow one another
    with pytest.raises(ValueError, match="one GPU"):
        M.frame_metrics(a, a)                                   # host tensors: there is no CPU path
