"""The TSRU recurrent unit in time: the frame-conditional training step with rnn="tsru" against rnn="gru", the recurrent stacks
of the generator in isolation with the TSRU's share split into its launches, and the new kernels' achieved bytes per second.

usage: python tools/tsru_step_time.py [--steps N] [--warmup W] [--batch B] [--ch C] [--frames T] [--n-cond K] [--size S]
                                      [--what step,stacks,kernels]
Prints one JSON line per measurement (HIP events around N repetitions after W warm-up ones, bf16):
  step      ms per train_step of a Trainer with config.n_cond = K, every Trainer in a child process of its own (--modes, default
            gru,tsru,gru,tsru: the units alternate and each is repeated, so the spread between processes is seen beside the
            difference), same seeds and clips; the summary gives each unit's runs and the range of tsru minus gru
  stack     per recurrent stack of the generator (frames of S/16, S/8, S/4, S/2 pixels; three layers): forward + backward of
            ConvTSRU.run and of ConvGRU.run on the same input, and the TSRU's time chain taken apart -- per layer T steps of
            {the two recurrent convolutions, the flow head, dvdx_tsru_forward} forward and {dvdx_tsru_backward, the flow head's
            and the two recurrent backward-data convolutions} backward, each timed alone back to back; "rest" = the stack minus
            those = x-part convolutions, weight gradients, weight packs and the gaps between launches
            (--trace-stack I:UNIT runs one stack of one unit alone, for a `rocprofv3 --kernel-trace` run: kernels against gaps)
  kernel    dvdx_tsru_forward / dvdx_tsru_backward at each stack's first-layer shape: LAUNCH-TO-LAUNCH ms (events around 50 calls
            back to back on the same buffers: at the small shapes the binding's launch floor, not the kernel; kernel time proper
            is a `rocprofv3 --kernel-trace --stats` run of this mode) and the bytes each must move at least (forward 14 bytes per
            element: h_prev 4, a_c + a_u 4, h 4, its copy 2; backward 36: dh + dh2 8, h_prev 4, a_c + a_u 4, da 4, g written 4
            and read 4, addend 4, dh_prev 4; the flow rows on top) over that time
"""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dvd_gan_amd import functional as Fn             # noqa: E402
from dvd_gan_amd import kern as K                     # noqa: E402
from dvd_gan_amd.train_step import Trainer           # noqa: E402

DEV = torch.device("cuda", 0)
BF = torch.bfloat16


def cfg(a):
    return argparse.Namespace(adv_loss="hinge", z_dim=120, g_chn=a.ch, ds_chn=a.ch, dt_chn=a.ch, n_frames=a.frames,
                              lr_schr="const", total_epoch=1, d_iters=1, batch_size=a.batch, g_lr=5e-5, d_lr=5e-5, beta1=0.0,
                              beta2=0.9, n_class=101, k_sample=8, n_cond=a.n_cond)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def step_time(a, rnn):
    torch.manual_seed(0)
    tr = Trainer([], cfg(a), device=DEV, compute_dtype=BF, latent_dim=a.size // 16, rnn=rnn, tsru_flow=a.flow)
    gen = torch.Generator().manual_seed(1)
    real = (torch.rand(a.batch, 3, a.n_cond + a.frames, a.size, a.size, generator=gen) * 2 - 1).to(DEV)
    labels = torch.randint(0, 101, (a.batch,), generator=gen).to(DEV)
    tr.register_label_buffer(labels)
    torch.manual_seed(100)
    ms = timed(lambda: tr.train_step(real, labels), a.steps, a.warmup)
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    del tr, real
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return ms, peak


def stages(a):
    """(frame side, input channels, hidden sizes, kernel sizes) of the generator's four recurrent stacks."""
    c8, c4, ld = 8 * a.ch, 4 * a.ch, a.size // 16
    return [(ld, c8, [c8, 2 * c8, c8], [3, 5, 3]), (2 * ld, c8, [c8, 2 * c8, c8], [3, 5, 3]),
            (4 * ld, c8, [c8, 2 * c8, c8], [3, 5, 3]), (8 * ld, c4, [c4, 2 * c4, c4], [3, 5, 5])]


def kernel_times(a, S, C, steps, warmup):
    """ms of one dvdx_tsru_forward and one dvdx_tsru_backward launch pair at [B, S, S, C], bf16 operands."""
    B = a.batch
    hp, dh, dh2, ad = (torch.randn(B, S, S, C, device=DEV) for _ in range(4))
    ag = torch.randn(B, S, S, 2 * C, device=DEV).to(BF)
    th = torch.randn(B, S, S, 8, device=DEV) * 0.5
    h, hc = torch.empty_like(hp), torch.empty(B, S, S, C, dtype=BF, device=DEV)
    da, dth, dhp = torch.empty_like(ag), torch.zeros(B, S, S, 8, dtype=BF, device=DEV), torch.empty_like(hp)
    ws = torch.empty(B * S * S * (C + 2), device=DEV)
    f = timed(lambda: Fn.tsru_forward(hp, ag, 0, C, th, a.flow, h, hc), steps, warmup)
    b = timed(lambda: Fn.tsru_backward(dh, dh2, hp, ag, 0, C, th, a.flow, da, 0, C, dth, ad, dhp, ws), steps, warmup)
    return f, b


def chain_times(a, S, C, k, steps, warmup):
    """ms of one step's launches of a TSRU layer at [B, S, S, C], each kind timed alone: (recurrent convs fwd, flow head fwd,
    flow head bwd-data, recurrent convs bwd-data)."""
    B, F_ = a.batch, Fn.tsru_flow_channels(C)
    mk = lambda c, dt=BF: torch.randn(B, S, S, c, device=DEV).to(dt)
    w = lambda co, ci, kk: torch.randn(co, ci, kk, kk, device=DEV) * 0.02
    phg = K.PackedConv(BF, 2 * C, C, (k, k), DEV, single_fill=True).fill(w(2 * C, C, k))
    phf = K.PackedConv(BF, F_, C, (k, k), DEV, single_fill=True).fill(w(F_, C, k))
    po = K.PackedConv(BF, 2, F_, (3, 3), DEV, single_fill=True).fill(w(2, F_, 3))
    h, gxg, gxf, af, dgg, dgf, dth = mk(C), mk(2 * C), mk(F_), mk(F_), mk(2 * C), mk(F_), mk(8)
    ag, af_o, th = torch.empty_like(gxg), torch.empty_like(gxf), torch.empty(B, S, S, 8, device=DEV)

    def rec_fwd():
        K.conv_forward(h, phg.wf, (k, k), 2 * C, res=gxg, out=ag, wq=lambda: phg.fragment_major("wf"))
        K.conv_forward(h, phf.wf, (k, k), F_, res=gxf, out=af_o, wq=lambda: phf.fragment_major("wf"))

    def rec_bwd():
        part = K.conv_forward(dgg, phg.wd, (k, k), phg.cip, wq=lambda: phg.fragment_major("wd"))
        K.conv_forward(dgf, phf.wd, (k, k), phf.cip, res=part, out_f32=True, wq=lambda: phf.fragment_major("wd"))

    head_fwd = lambda: K.conv_forward(af, po.wf, (3, 3), 2, relu_in=True, out=th, out_f32=True)
    head_bwd = lambda: K.conv_forward(dth, po.wd, (3, 3), po.cip, mask=af, out=dgf)
    return tuple(timed(fn, steps, warmup) for fn in (rec_fwd, head_fwd, head_bwd, rec_bwd))


def stack_times(a, stage, only=None):
    """only="tsru" / "gru": that stack's forward + backward alone and nothing else (what a kernel trace is taken of)."""
    from dvd_gan_amd.gen_net import ConvGRU, ConvTSRU
    S, cin, hidden, ks = stage
    T, B = a.frames, a.batch
    out = {"side": S, "hidden": hidden, "kernels": ks, "T": T, "B": B}
    torch.manual_seed(0)
    x = torch.randn(T * B, S, S, cin, device=DEV).to(BF).requires_grad_(True)
    h0 = [torch.randn(B, S, S, c, device=DEV).to(BF).requires_grad_(True) for c in hidden]
    for name, make in (("tsru", lambda: ConvTSRU(cin, hidden, ks, 3, flow=a.flow)), ("gru", lambda: ConvGRU(cin, hidden, ks, 3))):
        if only not in (None, name):
            continue
        net = make()
        net = net.to(DEV)
        if name == "tsru":
            for cell in net.cells:                  # a flow head off zero: the warp samples between pixels, as in a trained unit
                torch.nn.init.normal_(cell.flow_out.weight, std=0.05)

        def run():
            ys = net.run(x, T, False, h0)
            torch.autograd.backward([ys[-1]], [torch.ones_like(ys[-1])])
            x.grad = None
            for p in list(net.parameters()) + h0:
                p.grad = None
        out[f"{name}_fwd_bwd_ms"] = round(timed(run, a.steps, a.warmup), 3)
        del net
    if only is not None:
        return out
    new = rec = head = 0.0
    for C, k in zip(hidden, ks):
        f, b = kernel_times(a, S, C, 20, 5)
        rf, hf, hb, rb = chain_times(a, S, C, k, 20, 5)
        new += T * (f + b)
        rec += T * (rf + rb)
        head += T * (hf + hb)
    out.update(tsru_new_kernels_ms=round(new, 3), tsru_recurrent_convs_ms=round(rec, 3), tsru_flow_head_ms=round(head, 3),
               tsru_rest_ms=round(out["tsru_fwd_bwd_ms"] - new - rec - head, 3), launches_on_the_chain=3 * T * 9)
    torch.cuda.empty_cache()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--ch", type=int, default=32)
    p.add_argument("--frames", type=int, default=12)
    p.add_argument("--n-cond", type=int, default=4)
    p.add_argument("--size", type=int, default=128)
    p.add_argument("--flow", type=float, default=2.0)
    p.add_argument("--what", default="step,stacks,kernels")
    p.add_argument("--modes", default="gru,tsru,gru,tsru", help="Trainers to time, in this order (a name may repeat)")
    p.add_argument("--trace-stack", default="", metavar="I:UNIT",
                   help="only stack I (0..3) of UNIT (tsru | gru), forward + backward: the run to take a kernel trace of")
    p.add_argument("--one", default="", help=argparse.SUPPRESS)
    p.add_argument("--child-timeout", type=float, default=240.0)
    a = p.parse_args()
    if a.one:                                  # a child: one Trainer, one line
        ms, peak = step_time(a, a.one)
        print(json.dumps({"step": a.one, "ms_per_step": round(ms, 2), "peak_gb": round(peak, 1)}), flush=True)
        return
    if a.trace_stack:
        i, unit = a.trace_stack.split(":")
        print(json.dumps({"stack": stack_times(a, stages(a)[int(i)], only=unit)}), flush=True)
        return
    what = a.what.split(",")
    shape = f"B={a.batch}, K={a.n_cond}, T={a.frames}, {a.size}x{a.size}, ch={a.ch}, bf16, d={a.flow}"
    if "step" in what:
        # every Trainer in a process of its own, and before this process touches the device (tools/aug_step_time.py says why)
        res = {}
        for mode in a.modes.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", mode] + [
                f"--{k.replace('_', '-')}={getattr(a, k)}" for k in ("steps", "warmup", "batch", "ch", "frames", "n_cond", "size", "flow")]
            out = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.child_timeout, check=True).stdout.decode()
            row = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
            res.setdefault(mode, []).append(row["ms_per_step"])
            print(json.dumps(row), flush=True)
        g, t = res.get("gru"), res.get("tsru")
        print(json.dumps({"summary": {"gru_ms": g, "tsru_ms": t,
                                      "tsru_minus_gru_ms": None if not (g and t) else [round(min(t) - max(g), 2), round(max(t) - min(g), 2)],
                                      "shape": shape}}), flush=True)
    if "kernels" in what:
        for S, _, hidden, _ in stages(a):
            C = hidden[0]
            f, b = kernel_times(a, S, C, 50, 10)
            n = a.batch * S * S
            fb, bb = n * (14 * C + 32), n * (36 * C + 32 + 16 + 16)
            print(json.dumps({"kernel": {"B": a.batch, "side": S, "C": C, "forward_ms": round(f, 4), "backward_ms": round(b, 4),
                                         "forward_GBps": round(fb / f / 1e6, 1), "backward_GBps": round(bb / b / 1e6, 1)}}), flush=True)
    if "stacks" in what:
        for stage in stages(a):
            print(json.dumps({"stack": stack_times(a, stage)}), flush=True)


if __name__ == "__main__":
    main()
