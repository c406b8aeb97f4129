"""The G / D_s / D_t training step of trainer.py:213-307 on the HIP path.

`Trainer(data_loader, config)` keeps the reference's constructor, `build_model`, `select_opt_schr`,
`calc_loss`, `reset_grad`, `train` names and the exact step order:
    perm(real) -> z -> z_class -> perm(fake)            (CPU default generator, trainer.py:233-242)
    D_s(real) , D_s(fake.detach)  -> backward -> ds Adam
    D_t(real↓), D_t(fake↓.detach) -> backward -> dt Adam
    D_s(fake), D_t(fake↓) on the UPDATED discriminators -> relu(1 - out) -> backward -> g Adam
Frame-conditional video prediction (config.n_cond = K > 0, BASELINE configs[4]): the clips are K context frames followed by
n_frames targets; the generator encodes the context (cond_encoder.FrameEncoder), D_s judges target frames against generated
ones, D_t judges whole clips -- the real clip against [context | generated].
Differences that do not change results: the dead D weight-gradients of the generator step are not
computed; Adam is one fused launch per network; gradients are exchanged with RCCL (dist.py).
Beyond the reference: config.ema_decay > 0 keeps an exponential moving average of the generator's weights, updated inside the
generator's Adam launch (optim.FlatAdam); `ema_weights()` / `sample(use_ema=True)` / `predict(use_ema=True)` compute with it and
`save_models` writes it as `{step}_G_ema.pth`.  A frame-conditional Trainer also has `rollout()` (autoregressive prediction past
n_frames) and `evaluate_prediction()` (PSNR / SSIM curves over the horizon, mean and best of N sampled futures; metrics.py).
config.g_ortho = beta > 0 adds BigGAN's orthogonal regularizer (Brock et al. 2019, eq. 3) to the generator's gradient right before
its Adam launch (optim.FlatAdam(ortho=beta)): every trainable matrix of G except the class embedding and the conditional-norm
embeddings; `ortho_penalty` is the device scalar sum 1/2 ||offdiag(W W^T)||_F^2 of the last generator step.
config.g_clip_norm / d_clip_norm > 0 clip the gradient of G / of D_s and D_t (each network on its own) to that norm,
config.skip_nonfinite leaves a network's weights and Adam state untouched in a step whose gradient holds an inf or a NaN,
config.grad_log = R keeps the last R steps' norms -- all on the device (optim.FlatAdam's guard): `grad_norms` are device scalars,
`guard_report()` is the one call that reads them back.
config.sample_step = N > 0 (or the reference's sample_epoch) writes sample sheets every N steps (trainer.py:186,195-197,323-334):
`save_samples` runs eval-mode G on the fixed noise of `fixed_inputs()`, one HIP launch turns the clips into 8-bit sheets
(sheets.make_sheets) and a sheets.SheetWriter compresses and writes them on a worker thread -- one PNG per clip under the
reference's names, and / or one animated PNG of all clips (config.sample_layout).  `save_predictions` writes real-against-predicted
comparison sheets of a frame-conditional generator, `save_real` the loader's clips.  None of them leaves a trace in the training
state or in the default generator.
config.state_save_step = N > 0 writes the FULL training state every N steps (`save_state`: weights, Adam m / v / t, the weight
average, the guard's counters, schedules, random streams, loader position; `{step}_state.pt`, the newest config.state_keep kept)
behind the training loop (checkpoint.StateWriter), and config.resume = a state file or "latest" makes `train()` continue from it:
the continued run is bit-equal to the run that was never stopped.  `save_models` / config.pretrained_model remain the
reference-format, weights-only path.
config.lecam = lambda > 0 adds LeCam regularization (Tseng et al. 2021) to the discriminators' gradients, config.g_topk = nu > 0
lets the generator step take gradient only from the samples each discriminator scores highest (Sinha et al. 2020), config.d_stats
keeps logit statistics, among them the overfitting indicator r_t = E[sign D(real)] (Karras et al. 2020): all inside the loss
launch (functional.AdvLossEx), nothing read back; `d_stats()` is the one call that synchronizes.
config.d_aug = "color,translation,cutout" (any subset) transforms what the discriminators see, real and generated clips alike and
every frame of a clip alike (augment.py: Zhao et al. 2020, two HIP launches, the generator's gradient passes through the
transform); each group applies to a clip with probability config.d_aug_p, which config.d_aug_target > 0 steers by r_t every
config.d_aug_interval steps (Karras et al. 2020; `d_aug_p` is the current value).
config.d_aug_geom = "xflip,rot90,scale,rotate,aniso" (any subset) warps the clips before that: ADA's geometric group as one
affine map per clip, bilinear with zero fill (geom_augment.py: two more HIP launches, the warp and its exact transpose, no
atomics); it shares d_aug_p and its steering, d_aug_seed and the tables' generator with d_aug, and either works without the other.
`evaluate_samples(real, n_samples=N, embed=...)` measures generation from noise (n_cond = 0): the Frechet and the kernel distance
between features of real and of generated clips (distmetrics.py; the statistic of FVD / FID / KID, on the device).  `embed` is the
caller's feature extractor or "Dt" / "Ds", this Trainer's own discriminator features -- comparable only under ONE fixed
discriminator snapshot.  It leaves no trace in the training state or in any random stream.
Out of scope: tensorboard logging, GIF / MP4 files, dataset loaders.
"""
import contextlib
import os
import time

import torch

from . import functional as Fn
from . import kern as K
from . import lib as L
from . import dist as D
from .augment import ClipAugment, ada_update, draw_params, parse_policy
from .geom_augment import ClipWarp, draw_geom, parse_geom
from .dist import GradExchange
from .disc_nets import SpatialDiscriminator, TemporalDiscriminator
from .gen_net import Generator
from .helpers import (denorm, draw_frame_ids, sample_k_frames, to_device_async, truncated_z, vid_downsample,
                      vid_downsample_cat)
from .optim import FlatAdam


class _StepLR:
    """lr schedule arithmetic of trainer.py:142-176 ('const' | 'step' | 'exp' | 'multi')."""

    def __init__(self, opt, kind, base_lr):
        self.opt, self.kind, self.base, self.n = opt, kind, base_lr, 0

    def step(self, metric=None):
        self.n += 1
        n, lr = self.n, self.base
        if self.kind == "step":
            lr = self.base * 0.98 ** (n // 500)
        elif self.kind == "exp":
            lr = self.base * 0.9999 ** n
        elif self.kind == "multi":
            lr = self.base * 0.3 ** ((n >= 10000) + (n >= 30000))
        self.opt.param_groups[0]["lr"] = lr

    def get_lr(self):
        return [self.opt.param_groups[0]["lr"]]

    def state_dict(self):
        return {"kind": self.kind, "n": self.n, "lr": self.opt.param_groups[0]["lr"]}

    def load_state_dict(self, sd):
        if sd["kind"] != self.kind:
            raise ValueError(f"lr_schr: the state was written by a {sd['kind']!r} schedule, this one is {self.kind!r}")
        self.n = int(sd["n"])
        self.opt.param_groups[0]["lr"] = float(sd["lr"])


class _PlateauLR:
    """lr_schr='reduce' (trainer.py:158-176): ReduceLROnPlateau(mode='min', factor=lr_decay, patience=100,
    threshold=1e-4 'rel', cooldown=0, min_lr=1e-10, eps=1e-8) -- same arithmetic as torch's scheduler.  The reference
    calls `.step()` WITHOUT the metric (trainer.py:254,270,308), which raises TypeError at its first iteration, so that
    mode never ran there; here each network's scheduler is fed that network's loss of the step (what the configuration
    evidently intends).  Reading the loss costs one host sync per optimizer phase -- only in this mode."""

    def __init__(self, opt, factor, base_lr, patience=100, threshold=1e-4, min_lr=1e-10, eps=1e-8):
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        self.opt, self.factor, self.patience, self.threshold, self.min_lr, self.eps = opt, factor, patience, threshold, min_lr, eps
        self.best, self.bad = float("inf"), 0
        self.opt.param_groups[0]["lr"] = base_lr

    def step(self, metric):
        if metric is None:
            raise TypeError("step() missing 1 required positional argument: 'metrics'")
        if D.exchange_on():
            # data parallel: every rank must take the SAME lr decision or the replicas' parameters drift apart for good
            # (only gradients are exchanged) -- the schedulers see the mean of the ranks' losses.  (A Python float is accepted
            # like in the single-process path; every rank must call step() every iteration: it is a collective.)
            dev = metric.device if isinstance(metric, torch.Tensor) else D.collective_device()
            metric = torch.as_tensor(metric, dtype=torch.float32).detach().to(dev).clone().reshape(1)
            torch.distributed.all_reduce(metric, op=torch.distributed.ReduceOp.SUM)
            metric = metric / D.world_size()
        m = float(metric)
        if m < self.best * (1.0 - self.threshold):
            self.best, self.bad = m, 0
        else:
            self.bad += 1
        if self.bad > self.patience:
            old = self.opt.param_groups[0]["lr"]
            new = max(old * self.factor, self.min_lr)
            if old - new > self.eps:
                self.opt.param_groups[0]["lr"] = new
            self.bad = 0

    def get_lr(self):
        return [self.opt.param_groups[0]["lr"]]

    def state_dict(self):
        return {"kind": "reduce", "best": self.best, "bad": self.bad, "lr": self.opt.param_groups[0]["lr"]}

    def load_state_dict(self, sd):
        if sd["kind"] != "reduce":
            raise ValueError(f"lr_schr: the state was written by a {sd['kind']!r} schedule, this one is 'reduce'")
        self.best, self.bad = float(sd["best"]), int(sd["bad"])
        self.opt.param_groups[0]["lr"] = float(sd["lr"])


def topk_keep(batch, nu, gamma, epoch):
    """Samples the generator step keeps in `epoch` (0-based): max(ceil(nu * B), floor(B * gamma^epoch)), annealed from the whole
    batch down to the floor nu (Sinha et al. 2020), never below 1 or above B."""
    import math
    return max(1, min(int(batch), max(math.ceil(nu * batch), math.floor(batch * gamma ** epoch))))


class Trainer(object):
    def __init__(self, data_loader, config, device=None, compute_dtype=torch.bfloat16, latent_dim=4, dp_mode="replica"):
        """dp_mode (data-parallel runs only): "replica" = per-replica batch-norm statistics and condition rows, the
        semantics of the reference's nn.DataParallel (trainer.py:353-359); "global" = cross-replica conditional batch
        norm + gathered conditions: N ranks reproduce one process on the global batch."""
        if dp_mode not in ("replica", "global"):
            raise ValueError("dp_mode must be 'replica' or 'global'")
        self.dp_mode = dp_mode
        self.data_loader = data_loader
        c = self.config = config
        self.adv_loss, self.z_dim = c.adv_loss, c.z_dim
        self.g_chn, self.ds_chn, self.dt_chn = c.g_chn, c.ds_chn, c.dt_chn
        self.n_frames, self.lr_schr = c.n_frames, c.lr_schr
        self.total_epoch, self.d_iters, self.batch_size = c.total_epoch, c.d_iters, c.batch_size
        self.g_lr, self.d_lr, self.beta1, self.beta2 = c.g_lr, c.d_lr, c.beta1, c.beta2
        self.n_class, self.k_sample = c.n_class, c.k_sample
        self.n_cond = int(getattr(c, "n_cond", 0))
        if self.n_cond < 0:
            raise ValueError(f"n_cond={self.n_cond}")
        if self.n_cond and (self.n_cond + self.n_frames) % 4:
            # D_t sees context + generated frames and pools time twice (TemporalDiscriminator._forward)
            raise ValueError(f"n_cond + n_frames = {self.n_cond + self.n_frames} must be a multiple of 4: D_t judges the context "
                             "and the generated frames together and pools time twice")
        # generator weight average (0 = off): decay, steps it merely follows the weights, standing-statistics passes at
        # sampling / saving time and the seed of their private noise generator
        self.ema_decay = float(getattr(c, "ema_decay", 0.0))
        self.ema_start = int(getattr(c, "ema_start", 0))
        self.ema_standing_stats = int(getattr(c, "ema_standing_stats", 0))
        self.ema_stats_seed = int(getattr(c, "ema_stats_seed", 0))
        if not 0.0 <= self.ema_decay < 1.0 or self.ema_start < 0 or self.ema_standing_stats < 0:
            raise ValueError(f"ema_decay={self.ema_decay} (in [0, 1)), ema_start={self.ema_start}, "
                             f"ema_standing_stats={self.ema_standing_stats} (both >= 0)")
        # orthogonal regularization of the generator's matrices (0 = off): strength beta of g += beta * 2 M W
        self.g_ortho = float(getattr(c, "g_ortho", 0.0))
        if not 0.0 <= self.g_ortho < float("inf"):
            raise ValueError(f"g_ortho={self.g_ortho} must be a finite strength >= 0")
        # gradient guard (all 0 / False = off): clipping norms of G and of the two discriminators, skipping of non-finite steps,
        # rows of the per-network norm log
        self.g_clip_norm = float(getattr(c, "g_clip_norm", 0.0))
        self.d_clip_norm = float(getattr(c, "d_clip_norm", 0.0))
        self.skip_nonfinite = bool(getattr(c, "skip_nonfinite", False))
        self.grad_log = int(getattr(c, "grad_log", 0))
        if not (0.0 <= self.g_clip_norm < float("inf") and 0.0 <= self.d_clip_norm < float("inf")) or self.grad_log < 0:
            raise ValueError(f"g_clip_norm={self.g_clip_norm}, d_clip_norm={self.d_clip_norm} (finite norms >= 0), "
                             f"grad_log={self.grad_log} (rows >= 0)")
        # stabilisers and diagnostics on the discriminators' logits (all 0 / False = off: calc_loss is then the plain launch).
        # LeCam regularization: strength, decay of the logit anchors, first D iteration the gradient applies in (the anchors
        # accumulate from the first one); top-k generator updates: floor nu of the kept fraction, its decay per epoch; the
        # logit statistics behind d_stats()
        self.lecam = float(getattr(c, "lecam", 0.0))
        self.lecam_decay = float(getattr(c, "lecam_decay", 0.99))
        self.lecam_start = int(getattr(c, "lecam_start", 0))
        self.g_topk = float(getattr(c, "g_topk", 0.0))
        self.g_topk_decay = float(getattr(c, "g_topk_decay", 0.99))
        self._d_stats_on = bool(getattr(c, "d_stats", False))
        if (not 0.0 <= self.lecam < float("inf") or not 0.0 <= self.lecam_decay < 1.0 or self.lecam_start < 0
                or not 0.0 <= self.g_topk <= 1.0 or not 0.0 < self.g_topk_decay <= 1.0):
            raise ValueError(f"lecam={self.lecam} (finite, >= 0), lecam_decay={self.lecam_decay} (in [0, 1)), "
                             f"lecam_start={self.lecam_start} (>= 0), g_topk={self.g_topk} (in [0, 1]), "
                             f"g_topk_decay={self.g_topk_decay} (in (0, 1])")
        # augmentation of what the discriminators see (d_aug = "" = off: no table, no generator, no launch): the groups of
        # augment.POLICIES, the probability a group applies to a clip with, the r_t it is steered towards (0 = fixed p), steps
        # between two adjustments, thousands of real clips in which p crosses [0, 1], seed of the tables' private generator
        self.d_aug = parse_policy(getattr(c, "d_aug", "") or "")
        # ... and the geometric groups of geom_augment.GEOM_POLICIES, applied before them; every other setting is shared
        self.d_aug_geom = parse_geom(getattr(c, "d_aug_geom", "") or "")
        self.d_aug_p = float(getattr(c, "d_aug_p", 1.0))          # the current p: adaptive runs move it (d_aug_target > 0)
        self.d_aug_target = float(getattr(c, "d_aug_target", 0.0))
        self.d_aug_interval = int(getattr(c, "d_aug_interval", 4))
        self.d_aug_kimg = float(getattr(c, "d_aug_kimg", 500))
        self.d_aug_seed = int(getattr(c, "d_aug_seed", 0))
        if (not 0.0 <= self.d_aug_p <= 1.0 or not 0.0 <= self.d_aug_target < 1.0 or self.d_aug_interval < 1
                or not 0.0 < self.d_aug_kimg < float("inf")):
            raise ValueError(f"d_aug_p={self.d_aug_p} (in [0, 1]), d_aug_target={self.d_aug_target} (in [0, 1), 0 = fixed p), "
                             f"d_aug_interval={self.d_aug_interval} (>= 1), d_aug_kimg={self.d_aug_kimg} (finite, > 0)")
        self._aug_adaptive = bool(self.d_aug or self.d_aug_geom) and self.d_aug_target > 0.0
        self._aug_gen = None          # the tables' generator, made below once the rank is known
        self._aug_steps = 0           # steps taken with d_aug or d_aug_geom on
        self._aug_adjustments = 0     # adjustments of p made
        self._adv_ex = self.lecam > 0.0 or self.g_topk > 0.0 or self._d_stats_on or self._aug_adaptive
        self._anchors = None          # fp32 [2 slots][D_s, D_t][real, fake] on the device, when lecam > 0
        self._adv_stats = None        # fp32 [6][lib.ADV_NSTAT]: D_s real / fake, D_t real / fake, G step D_s / D_t
        self._lecam_it = 0            # D iterations done
        # singular-value monitoring of the weights (sv_log = 0 = off: no table, no workspace, no launch): every sv_log-th step
        # sv_iters more block power iterations on each network's monitor and one row of its device ring of sv_log_rows rows; top
        # sv_k values from blocks of sv_block columns, start blocks from a private generator seeded with sv_seed (spectral.py)
        self.sv_log = int(getattr(c, "sv_log", 0) or 0)
        self.sv_iters = int(getattr(c, "sv_iters", 4))
        self.sv_log_rows = int(getattr(c, "sv_log_rows", 64))
        self.sv_k = int(getattr(c, "sv_k", 3))
        self.sv_block = int(getattr(c, "sv_block", 8))
        self.sv_seed = int(getattr(c, "sv_seed", 0))
        if (self.sv_log < 0 or not 1 <= self.sv_iters <= L.SV_MAX_ITERS or self.sv_log_rows < 1
                or not 1 <= self.sv_k <= self.sv_block <= L.SV_MAX_BLOCK):
            raise ValueError(f"sv_log={self.sv_log} (>= 0), sv_iters={self.sv_iters} (in [1, {L.SV_MAX_ITERS}]), "
                             f"sv_log_rows={self.sv_log_rows} (>= 1), sv_k={self.sv_k}, sv_block={self.sv_block} "
                             f"(1 <= sv_k <= sv_block <= {L.SV_MAX_BLOCK})")
        self._sv = None               # {"G", "Ds", "Dt"} -> spectral.SpectrumMonitor, made at first use
        self._sv_steps = 0            # steps this Trainer has taken
        self._sv_logged = []          # step numbers of the rows logged so far
        self.lr_decay = getattr(c, "lr_decay", 0.9999)
        self.pretrained_model = getattr(c, "pretrained_model", None)
        self.model_save_path = os.path.join(getattr(c, "model_save_path", "./models"), getattr(c, "version", ""))
        self.model_save_epoch = getattr(c, "model_save_epoch", 0)
        self.log_epoch = getattr(c, "log_epoch", 1)
        # exact resume (all unset = off: no thread, no allocation, no file): a full training state every state_save_step steps
        # as `{step}_state.pt`, the newest state_keep of them kept (0 = all); resume = a state file or "latest"
        self.state_save_step = int(getattr(c, "state_save_step", 0) or 0)
        self.state_keep = int(getattr(c, "state_keep", 2))
        self.resume = getattr(c, "resume", None) or None
        if self.state_save_step < 0 or self.state_keep < 0:
            raise ValueError(f"state_save_step={self.state_save_step}, state_keep={self.state_keep} (both >= 0)")
        if self.resume and self.pretrained_model:
            raise ValueError(f"resume={self.resume!r} and pretrained_model={self.pretrained_model!r}: a run continues either from a "
                             "full training state or from reference-format weights, not from both")
        self._state_writer = None     # the checkpoint.StateWriter, made at the first save_state()
        self._resumed_step = None     # the step of the state load_state() read
        # sample sheets (sample_step = sample_epoch = 0: off): period in steps, or in epochs like the reference (trainer.py:186);
        # directory (trainer.py:69); clips per class; "frames" = a PNG per clip, "clips" = one animation of all clips, "both"
        self.sample_step = int(getattr(c, "sample_step", 0) or 0)
        self.sample_epoch = getattr(c, "sample_epoch", 0) or 0
        self.sample_path = os.path.join(getattr(c, "sample_path", "./samples"), getattr(c, "version", ""))
        self.test_batch_size = int(getattr(c, "test_batch_size", 8))
        self.sample_layout = getattr(c, "sample_layout", "frames")
        self.sample_fps = getattr(c, "sample_fps", 8)
        self.sample_use_ema = bool(getattr(c, "sample_use_ema", False))
        self.sample_seed = int(getattr(c, "sample_seed", 0))
        if (self.sample_step < 0 or self.sample_epoch < 0 or self.test_batch_size < 1 or not self.sample_fps > 0
                or self.sample_layout not in ("frames", "clips", "both")):
            raise ValueError(f"sample_step={self.sample_step}, sample_epoch={self.sample_epoch} (>= 0), "
                             f"test_batch_size={self.test_batch_size} (>= 1), sample_fps={self.sample_fps} (> 0), "
                             f"sample_layout={self.sample_layout!r} ('frames' | 'clips' | 'both')")
        self._fixed = None            # fixed_inputs(), drawn at first use
        self._sheets = None           # the sheets.SheetWriter, made at first use
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.compute_dtype, self.latent_dim = compute_dtype, latent_dim
        if self._adv_ex:
            self._adv_stats = torch.zeros(6, L.ADV_NSTAT, dtype=torch.float32, device=self.device)
            if self.lecam > 0.0:
                self._anchors = torch.zeros(2, 2, 2, dtype=torch.float32, device=self.device)
        Fn.direct_weight_grads(True)          # weight gradients accumulate into FlatAdam's buffers on a side stream
        self.exchange = GradExchange()
        # The step's dependent chain runs on a high-priority stream (ahead of the bulk weight-gradient stream) -- in a
        # single-process run.  In a data-parallel run the gradient exchange takes the urgent level instead and the chain
        # stays on the caller's stream, so RCCL's kernels are not queued behind every launch of the step while an exchange
        # is pending.  DVD_CHAIN_PRIO=1 / 0 forces the high-priority chain on / off.
        prio = os.environ.get("DVD_CHAIN_PRIO", "auto")
        self._chain = None
        self._aux = None          # stream of the discriminator passes over the real clips (see _train_step)
        if torch.cuda.is_available() and (prio == "1" or (prio == "auto" and not self.exchange.active)):
            self._chain = torch.cuda.Stream(priority=torch.cuda.Stream.priority_range()[1])
            # opt-in: -1.6 ms of 537 at 64 x 64, but the step DOUBLES at 48 x 128 x 128 (2002 -> 4043 ms; 175 GB of activations: blocks
            # freed on the second stream are not reusable by the first and the allocator falls back to synchronising frees)
            if not self.exchange.active and os.environ.get("DVD_D_REAL_EARLY", "0") == "1":
                self._aux = torch.cuda.Stream()
        self.rank = torch.distributed.get_rank() if self.exchange.active else 0
        if self.d_aug or self.d_aug_geom:
            if self._aug_adaptive and self.exchange.active:
                raise ValueError(f"d_aug_target={self.d_aug_target}: an adaptive augmentation probability is not served in a "
                                 "data-parallel run (every rank would have to agree on p); use a fixed d_aug_p")
            self._aug_gen = self._new_aug_gen()
        self.build_model()
        if self.pretrained_model:
            self.load_pretrained_model()
        # data parallel: every rank continues from rank 0's model (parameters, SN u / v, BN statistics); frame ids come
        # from a generator all ranks seed alike, z / labels from each rank's own default generator
        self._sync_replicas()
        self.frame_gen = torch.Generator().manual_seed(D.shared_seed()) if self.exchange.active else None
        # ... and z / z_class of rank r from a generator of its own: distinct noise per replica even when every rank was
        # seeded alike (equal seeds on all ranks would train every replica on the same draws).  Its seed mixes the rank with
        # config.seed when the configuration has one, else with a value DRAWN from the caller's default generator -- so
        # torch.manual_seed(...) before constructing the Trainer steers it, two runs with different seeds draw different
        # noise, and a resumed run (which re-seeds or not as the caller likes) does not replay a fixed stream.
        # A single process keeps the default generator -- the reference's behaviour (trainer.py:84-88, 236-240).
        self.noise_gen = None
        if self.exchange.active:
            base = getattr(c, "seed", None)
            if base is None:
                base = int(torch.randint(0, 2 ** 31 - 1, (1,)))
            self.noise_gen = torch.Generator().manual_seed((int(base) * 1000003 + 7919 * self.rank + 1) % (2 ** 63 - 1))

    def _new_aug_gen(self):
        """The private generator of the augmentation tables: d_aug_seed, mixed with the rank in a data-parallel run as noise_gen's
        seed is.  Neither the default generator nor noise_gen is touched by a table."""
        seed = self.d_aug_seed
        if self.exchange.active:
            seed = (int(seed) * 1000003 + 7919 * self.rank + 1) % (2 ** 63 - 1)
        return torch.Generator().manual_seed(seed)

    def _aug_table(self, draws, key, B, H, W):
        """One parameter table [B, lib.AUG_COLS] on the device: draws[key] (test aid) or a draw from the private generator."""
        if draws is not None and key in draws:
            tab = torch.as_tensor(draws[key], dtype=torch.float32).reshape(B, L.AUG_COLS).contiguous()
        else:
            tab = draw_params(B, H, W, self.d_aug, self.d_aug_p, self._aug_gen)
        return to_device_async(tab, self.device)

    def _geom_table(self, draws, key, B, H, W):
        """One table of warps [B, lib.GEOM_COLS] on the device: draws[key] (test aid) or a draw from the private generator."""
        if draws is not None and key in draws:
            tab = torch.as_tensor(draws[key], dtype=torch.float32).reshape(B, L.GEOM_COLS).contiguous()
        else:
            tab = draw_geom(B, H, W, self.d_aug_geom, self.d_aug_p, self._aug_gen)
        return to_device_async(tab, self.device)

    @staticmethod
    def _d_view(clips, mats, tab):
        """What the discriminators are given of `clips` [B, T, 3, H, W]: the warp first, then colour / translation / cutout
        (Karras et al. 2020's order); a table that is None is a stage that is off."""
        if mats is not None:
            clips = ClipWarp.apply(clips, mats)
        if tab is not None:
            clips = ClipAugment.apply(clips, tab)
        return clips

    def _aug_adapt(self):
        """After every d_aug_interval-th step: p follows the sign of r_t - d_aug_target, r_t the mean of the two discriminators'
        E[sign D(real)] of this step (one synchronizing read of two floats)."""
        self._aug_steps += 1
        if not self._aug_adaptive or self._aug_steps % self.d_aug_interval:
            return
        r = self._adv_stats[:, L.ADV_STAT_SIGN].cpu().tolist()
        self.d_aug_p = ada_update(self.d_aug_p, 0.5 * (r[0] + r[2]), self.d_aug_target, self.batch_size, self.d_aug_interval,
                                  self.d_aug_kimg)
        self._aug_adjustments += 1

    # ---- trainer.py:345-366
    def build_model(self):
        dt = self.compute_dtype
        c = self.config
        self.G = Generator(self.z_dim, self.latent_dim, self.n_class, self.g_chn, self.n_frames, compute_dtype=dt,
                           self_attn=getattr(c, "g_self_attn", False), sep_attn=getattr(c, "g_sep_attn", False),
                           n_cond=self.n_cond).to(self.device)
        self.D_s = SpatialDiscriminator(self.ds_chn, self.n_class, compute_dtype=dt).to(self.device)
        self.D_t = TemporalDiscriminator(self.dt_chn, self.n_class, compute_dtype=dt).to(self.device)
        if self.exchange.active and self.dp_mode == "global":
            from .sn_layers import ConditionalNorm
            self.G.dp_global = True
            for m in self.G.modules():
                if isinstance(m, ConditionalNorm):
                    m.replicas = (self.exchange.world, D.all_reduce_sum_)
        self.select_opt_schr()

    @property
    def ortho_penalty(self):
        """Device scalar (float64): sum over the regularised matrices of 1/2 ||offdiag(W W^T)||_F^2, on the weights the last
        generator step started from, unscaled; None when config.g_ortho = 0 or before the first step."""
        return self.g_optimizer.ortho_penalty

    def _optimizers(self):
        return (("G", self.g_optimizer), ("Ds", self.ds_optimizer), ("Dt", self.dt_optimizer))

    @property
    def grad_norms(self):
        """{"G", "Ds", "Dt"} -> device scalar (float64): the norm of the finite part of the gradient that network's last Adam
        launch consumed (None for a network whose guard is off or that has not stepped yet).  None when no guard is configured.
        Reading an entry on the host synchronizes; nothing here does."""
        if not any(opt.guard for _, opt in self._optimizers()):
            return None
        return {tag: opt.grad_norm for tag, opt in self._optimizers()}

    def guard_report(self):
        """{"G", "Ds", "Dt"} -> host dict (optim.FlatAdam.guard_report: norm, coef, bad, skip, seen, skipped, clipped, ring rows in
        step order; None for a network without a guard).  The only call of the guard that synchronizes.  None when no guard is
        configured."""
        if not any(opt.guard for _, opt in self._optimizers()):
            return None
        return {tag: opt.guard_report() for tag, opt in self._optimizers()}

    # ---- singular values of the weights (spectral.py)
    def _sv_monitors(self):
        """One monitor per network over every trainable tensor with dim() >= 2 (named by its state_dict key), with the layer's
        weight_u / weight_v where it is spectrally normalised.  The ring's last row is sv_report()'s own."""
        if self._sv is None:
            from .spectral import SpectrumMonitor
            self._sv = {}
            for tag, net in (("G", self.G), ("Ds", self.D_s), ("Dt", self.D_t)):
                prm = dict(net.named_parameters())
                mats = [(n, p.data) for n, p in prm.items() if p.requires_grad and p.dim() >= 2]
                sn = {}
                for n, _ in mats:
                    stem = n[:-len("weight_bar")] if n.endswith("weight_bar") else None
                    if stem is not None and stem + "weight_u" in prm and stem + "weight_v" in prm:
                        sn[n] = (prm[stem + "weight_u"].data, prm[stem + "weight_v"].data)
                self._sv[tag] = SpectrumMonitor(mats, k=self.sv_k, block=self.sv_block, seed=self.sv_seed, sn=sn,
                                                rows=self.sv_log_rows + 1)
        return self._sv

    def _sv_log_row(self):
        row = len(self._sv_logged) % self.sv_log_rows
        for mon in self._sv_monitors().values():
            mon.update(self.sv_iters).snapshot(row)
        self._sv_logged.append(self._sv_steps)

    def sv_report(self, iters=None, reset=False):
        """{"G", "Ds", "Dt"} -> list of {name, shape, sv, res, stable_rank, sn_sigma}, one entry per trainable tensor with
        dim() >= 2: the top sv_k singular values of the tensor viewed [shape[0], -1] after `iters` (default config.sv_iters) more
        iterations from the blocks the monitors hold (reset=True: from the seeded start blocks), their residuals, the stable rank
        |W|_F^2 / sv[0]^2 and, for a spectrally normalised layer, sn_sigma = u^T W v of its weight_u / weight_v (else None):
        sv[0] / sn_sigma says how far the normalisation lags behind the weights.  The values are Ritz values: lower bounds that
        rise towards the singular values as the block converges (error ~ (sigma_{b+1} / sigma_i)^(2 iterations)), and for each of
        them some singular value of W (or 0) lies within its `res`; see spectral.py.  The one call of this group that
        synchronizes; works with sv_log = 0 too (the monitors are built at first use).  Reads the weights in place and changes
        nothing: not the weights, the optimizer state, weight_u / weight_v, batch-norm statistics or any random stream.  The
        blocks and the ring are a log, not training state: they are not in the state file, a resumed run starts them afresh."""
        iters = self.sv_iters if iters is None else int(iters)
        if iters < 0:
            raise ValueError(f"iters={iters}")
        mons = self._sv_monitors()
        for mon in mons.values():
            if reset:
                mon.reset()
            mon.update(iters).snapshot(self.sv_log_rows)
        out = {}
        for tag, mon in mons.items():
            sv, res, fro2, sn = (t.tolist() for t in mon.split(mon.ring[self.sv_log_rows].cpu()))
            out[tag] = [{"name": n, "shape": tuple(t.shape), "sv": sv[i], "res": res[i],
                         "stable_rank": fro2[i] / sv[i][0] ** 2 if sv[i][0] > 0.0 else float("nan"),
                         "sn_sigma": sn[i] if mon.sn[i] is not None else None}
                        for i, (n, t) in enumerate(zip(mon.names, mon.tensors))]
        return out

    def sv_history(self):
        """The rows config.sv_log has written, oldest first (the newest sv_log_rows of them): {"steps": [step of each row, counted
        from this Trainer's first step = 1], "G" / "Ds" / "Dt": {"names", "sv" [rows, n, k], "res" [rows, n, k], "fro2" [rows, n],
        "sn_sigma" [rows, n] (NaN without spectral norm)}} as host tensors.  Synchronizes.  None before the first logged row."""
        if self._sv is None or not self._sv_logged:
            return None
        count, cap = len(self._sv_logged), self.sv_log_rows
        order = [i % cap for i in range(max(0, count - cap), count)]
        out = {"steps": self._sv_logged[-cap:]}
        for tag, mon in self._sv.items():
            rows, k = mon.ring[:cap].cpu()[order], mon.k
            out[tag] = {"names": list(mon.names), "sv": rows[..., :k].contiguous(), "res": rows[..., k:2 * k].contiguous(),
                        "fro2": rows[..., 2 * k].contiguous(), "sn_sigma": rows[..., 2 * k + 1].contiguous()}
        return out

    def _sync_replicas(self):
        D.broadcast_state((self.G, self.D_s, self.D_t),
                          (self.g_optimizer.flat, self.ds_optimizer.flat, self.dt_optimizer.flat))

    # ---- trainer.py:134-176
    def select_opt_schr(self):
        betas = (self.beta1, self.beta2)
        guard = dict(skip_nonfinite=self.skip_nonfinite, norm_log=self.grad_log)
        self.g_optimizer = FlatAdam(self.G.parameters(), self.g_lr, betas, ema_decay=self.ema_decay, ema_start=self.ema_start,
                                    ortho=self.g_ortho, ortho_exclude=self.G.ortho_exclude() if self.g_ortho else (),
                                    clip_norm=self.g_clip_norm, **guard)
        # (the optional attention blocks and the conditioning encoder sit at the END of the parameter order but finish their
        #  gradients late in the backward pass -- the encoder's last of all, behind the dh0 of the first ConvGRU: with them the
        #  generator's gradient goes in one piece)
        self.G.dp_hooks = self.exchange.active and os.environ.get("DVD_DP_HOOKS", "1") != "0" and not (
            hasattr(self.G, "self_attn") or hasattr(self.G, "sep_attn") or hasattr(self.G, "cond_encoder"))
        # offset of the first trainable parameter of generator module conv.k in the flat buffers (gradient buckets)
        self._g_bounds, off = {}, 0
        for name, prm in self.G.named_parameters():
            if not prm.requires_grad:
                continue
            if name.startswith("conv."):
                self._g_bounds.setdefault(int(name.split(".")[1]), off)
            off += prm.numel()
        self.ds_optimizer = FlatAdam(self.D_s.parameters(), self.d_lr, betas, clip_norm=self.d_clip_norm, **guard)
        self.dt_optimizer = FlatAdam(self.D_t.parameters(), self.d_lr, betas, clip_norm=self.d_clip_norm, **guard)
        if self.lr_schr in ("const", "step", "exp", "multi"):
            self.g_lr_scher = _StepLR(self.g_optimizer, self.lr_schr, self.g_lr)
            self.ds_lr_scher = _StepLR(self.ds_optimizer, self.lr_schr, self.d_lr)
            self.dt_lr_scher = _StepLR(self.dt_optimizer, self.lr_schr, self.d_lr)
        else:                                   # trainer.py:158-176: anything else selects ReduceLROnPlateau
            self.g_lr_scher = _PlateauLR(self.g_optimizer, self.lr_decay, self.g_lr)
            self.ds_lr_scher = _PlateauLR(self.ds_optimizer, self.lr_decay, self.d_lr)
            self.dt_lr_scher = _PlateauLR(self.dt_optimizer, self.lr_decay, self.d_lr)
        self._plateau = not isinstance(self.g_lr_scher, _StepLR)

    # ---- trainer.py:114-121
    def calc_loss(self, x, real_flag, _site=None):
        """_site (passed by _train_step alone, and only when a stabiliser or the statistics are on): row of the statistics
        table -- 0 / 1 D_s real / fake, 2 / 3 D_t real / fake, 4 / 5 the generator step's D_s / D_t."""
        if _site is None or not getattr(self, "_adv_ex", False):
            return Fn.AdvLoss.apply(x, bool(real_flag), self.adv_loss == "hinge")
        group = x.numel() // self._cur_B               # k_sample for D_s, frames / 4 for D_t: the logits are sample-major
        keep, lecam, anchors = 0, 0.0, None
        if _site >= 4:
            if self.g_topk > 0.0:                      # (train() counts the epochs it has started: the running one is _epoch - 1)
                keep = topk_keep(self._cur_B, self.g_topk, self.g_topk_decay, max(0, getattr(self, "_epoch", 0) - 1))
                keep = 0 if keep >= self._cur_B else keep          # the whole batch: the same arithmetic without the ranking
        elif self._anchors is not None:
            # iteration `it` reads the anchors of slot (it - 1) & 1 and writes slot it & 1: the real and the fake call of a network
            # touch different floats and neither depends on the other's order (the real pass may run early on a side stream)
            it, net, kind = self._lecam_it, _site // 2, _site % 2
            prev, cur = self._anchors[(it - 1) & 1, net], self._anchors[it & 1, net]
            anchors = (prev[1 - kind:2 - kind], prev[kind:kind + 1], cur[kind:kind + 1], self.lecam_decay if it else 0.0)
            lecam = self.lecam if it >= self.lecam_start else 0.0
        return Fn.AdvLossEx.apply(x, bool(real_flag), self.adv_loss == "hinge", group, keep, lecam, anchors,
                                  self._adv_stats[_site])

    def _site_loss(self, x, real_flag, site):
        return self.calc_loss(x, real_flag, _site=site) if getattr(self, "_adv_ex", False) else self.calc_loss(x, real_flag)

    def _end_d_iteration(self):
        """The anchors of the slot this D iteration wrote become those of the global batch (the update is linear in the batch
        mean and the shards are equal): one all-reduce of 4 floats, only in a data-parallel run."""
        if getattr(self, "_anchors", None) is None:
            return
        if self.exchange.active:
            cur = self._anchors[self._lecam_it & 1]
            buf = cur.to(D.collective_device())
            torch.distributed.all_reduce(buf, op=torch.distributed.ReduceOp.SUM)
            cur.copy_(buf / D.world_size())
        self._lecam_it += 1

    def d_stats(self):
        """The logit statistics of the last step as a host dict, or None when lecam, g_topk and d_stats are all off.  The one
        call of this group that synchronizes.  Per discriminator: r_t = E[sign D(real)] (Karras et al. 2020: near 1 means D has
        memorised the training set), the mean logits, the hinge-active fractions, the LeCam penalties and the anchors they were
        measured against, the count of non-finite logits; and the samples the generator step kept."""
        if self._adv_stats is None:
            return None
        s = self._adv_stats.cpu().tolist()
        a = None if self._anchors is None else self._anchors[(self._lecam_it - 1) & 1].cpu().tolist()
        out = {"it": self._lecam_it}
        for net, tag in enumerate(("Ds", "Dt")):
            real, fake, g = s[2 * net], s[2 * net + 1], s[4 + net]
            out[tag] = {"r_t": real[L.ADV_STAT_SIGN], "sign_fake": fake[L.ADV_STAT_SIGN],
                        "mean_real": real[L.ADV_STAT_MEAN], "mean_fake": fake[L.ADV_STAT_MEAN],
                        "active_real": real[L.ADV_STAT_ACTIVE], "active_fake": fake[L.ADV_STAT_ACTIVE],
                        "lecam_real": real[L.ADV_STAT_LECAM], "lecam_fake": fake[L.ADV_STAT_LECAM],
                        "anchor_real": None if a is None else a[net][0], "anchor_fake": None if a is None else a[net][1],
                        "nonfinite": real[L.ADV_STAT_NONFINITE] + fake[L.ADV_STAT_NONFINITE] + g[L.ADV_STAT_NONFINITE],
                        "g_kept": int(g[L.ADV_STAT_KEPT]), "g_mean": g[L.ADV_STAT_MEAN]}
        return out

    # ---- trainer.py:84-88
    def label_sample(self):
        return to_device_async(torch.randint(low=0, high=self.n_class, size=(self.batch_size,), generator=self.noise_gen), self.device)

    # ---- trainer.py:384-387
    def reset_grad(self):
        self.ds_optimizer.zero_grad()
        self.dt_optimizer.zero_grad()
        self.g_optimizer.zero_grad()

    def _freeze_d(self, flag):
        self.D_s._set_train_weights(not flag)
        self.D_t._set_train_weights(not flag)

    # ---- trainer.py:223-307, one iteration (d_iters D updates + one G update)
    def _check_labels(self, labels):
        """Class ids index embedding tables on the device (no bounds check there): reject a label outside
        [0, n_class) while it is still on the host, like the IndexError nn.Embedding raises in the reference."""
        if not labels.numel():
            return labels
        if labels.is_cuda and getattr(self, "_labels_registered", None) is labels and self._labels_version == labels._version:
            return labels           # a buffer the caller registered as persistent and has not written since (bench.py)
        # (a device tensor costs a host sync to inspect -- labels normally arrive on the host (DataLoader, label_sample)
        #  and take the free path; nothing is cached by address: a fresh tensor can reuse a freed block)
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0 or hi >= self.n_class:
            raise IndexError(f"class id out of range for n_class={self.n_class}: [{lo}, {hi}]")
        return labels

    def register_label_buffer(self, labels):
        """Declare a DEVICE label tensor the caller re-uses unchanged every step: it is validated now and not again while
        its version counter stands (saves the host sync of the range check in a steady-state loop)."""
        self._labels_registered = None
        self._check_labels(labels)
        self._labels_registered, self._labels_version = labels, labels._version

    def train_step(self, real_videos, real_labels, draws=None, hidden=None):
        """real_videos [B,3,T,H,W], real_labels [B].  `draws` (tests): dict with the reference's RNG
        draws perm_real / z / z_class / perm_fake.  `hidden`: initial ConvGRU states for the generator
        (Generator.forward, frame-conditional variant).  With n_cond = K > 0 the clips are [B,3,K+T,H,W]: the first K frames
        condition the generator (`hidden` is then an error), perm_real / perm_fake draw over the T target frames, D_t sees
        all K+T frames.  Returns the six loss terms as device scalars:
        ds_real, ds_fake, dt_real, dt_fake, g_s, g_t.
        The step's dependent chain runs on a HIGH-priority stream so its (often small) launches are dispatched ahead of
        the bulk weight-gradient work queued on the normal-priority side stream; the caller's stream is ordered before
        and after the step, so nothing changes for it."""
        if self.n_cond:
            if hidden is not None:
                raise ValueError("a frame-conditional Trainer (n_cond > 0) takes its generator states from the context frames, "
                                 "not from `hidden`")
            if real_videos.dim() != 5 or real_videos.shape[2] != self.n_cond + self.n_frames:
                raise ValueError(f"clips must be [B, 3, n_cond + n_frames = {self.n_cond + self.n_frames}, H, W], got "
                                 f"{tuple(real_videos.shape)}")
        if self._chain is None:
            return self._train_step(real_videos, real_labels, draws, hidden)
        outer = torch.cuda.current_stream()
        self._chain.wait_stream(outer)
        with torch.cuda.stream(self._chain):
            out = self._train_step(real_videos, real_labels, draws, hidden)
        outer.wait_stream(self._chain)
        for v in out:
            v.record_stream(outer)
        return out

    def _train_step(self, real_videos, real_labels, draws=None, hidden=None):
        L.reset_gru_tickets(current_stream_only=True)         # split-K tickets start every step from zero (lib.reset_gru_tickets)
        real_videos = to_device_async(real_videos, self.device).permute(0, 2, 1, 3, 4).contiguous()
        real_labels = to_device_async(self._check_labels(real_labels), self.device)
        T, k, Kc = self.n_frames, self.k_sample, self.n_cond
        self._cur_B = real_videos.shape[0]
        cond = real_videos[:, :Kc].contiguous() if Kc else None       # [B,K,3,H,W] context frames; the targets follow them
        ex = self.exchange
        fg = self.frame_gen
        draws_all = draws
        aug, geo = bool(getattr(self, "d_aug", ())), bool(getattr(self, "d_aug_geom", ()))
        tab_real = tab_fake = mat_real = mat_fake = None
        for _ in range(self.d_iters):
            if isinstance(draws_all, (list, tuple)):              # test aid: one dict of draws per discriminator iteration
                draws = draws_all[_]
            ids_real = draw_frame_ids(T, k, fg) if draws is None else torch.as_tensor(draws["perm_real"])[:k].sort()[0]
            early = self._aux is not None
            real_in = real_videos
            if aug:
                # one table for the real clips and an independent one for the fake clips; both discriminators see the same
                # transform of a clip (the frame gather and the 2 x 2 average work on the augmented clip)
                tab_real = self._aug_table(draws, "aug_real", real_videos.shape[0], *real_videos.shape[-2:])
                tab_fake = self._aug_table(draws, "aug_fake", self.batch_size if draws is None else len(draws["z"]),
                                           *real_videos.shape[-2:])
            if geo:
                # the warps' tables come after those: a run without d_aug_geom draws what it drew before
                mat_real = self._geom_table(draws, "geom_real", real_videos.shape[0], *real_videos.shape[-2:])
                mat_fake = self._geom_table(draws, "geom_fake", self.batch_size if draws is None else len(draws["z"]),
                                            *real_videos.shape[-2:])
            if (aug or geo) and not early:
                real_in = self._d_view(real_videos, mat_real, tab_real)
            if not ((aug or geo) and early):
                real_s = sample_k_frames(real_in, T + Kc, k, ids_real + Kc if Kc else ids_real)
            z = to_device_async(torch.randn(self.batch_size, self.z_dim, generator=self.noise_gen) if draws is None
                                else torch.as_tensor(draws["z"]), self.device)
            z_class = self.label_sample() if draws is None else to_device_async(self._check_labels(torch.as_tensor(draws["z_class"])), self.device)
            ex.finish("G")
            if early:
                # The discriminator passes over the REAL clips need nothing from the generator: they run on a second stream beside
                # the 4 x 4 / 8 x 8 time loops at the start of the generator forward, the one phase of the step with idle CUs and
                # no weight-gradient work to fill them.  Same arithmetic in the same per-network order (real before fake, so the
                # spectral-norm state advances as in the reference); autograd runs their backward nodes on that stream too.
                cur = torch.cuda.current_stream()
                self._aux.wait_stream(cur)
                with torch.cuda.stream(self._aux):
                    if aug or geo:
                        # (real_in / real_s are allocated on this stream, like real_d: the weight-gradient launches that read
                        #  them on the side stream are fenced by Fn.join_side() before the step ends, and the next step's
                        #  wait_stream orders this stream behind the chain before any block can be reused)
                        real_in = self._d_view(real_videos, mat_real, tab_real)
                        real_s = sample_k_frames(real_in, T + Kc, k, ids_real + Kc if Kc else ids_real)
                    ds_loss_real = self._site_loss(self.D_s(real_s, real_labels), True, 0)
                    real_d = vid_downsample(real_in)
                    dt_loss_real = self._site_loss(self.D_t(real_d, real_labels), True, 2)
                for t_ in (real_videos, real_labels) + (tuple(t for t in (tab_real, mat_real) if t is not None) or (real_s,)):
                    t_.record_stream(self._aux)
            fake_videos = self.G(z, z_class, hidden, cond=cond)
            ids_fake = draw_frame_ids(T, k, fg) if draws is None else torch.as_tensor(draws["perm_fake"])[:k].sort()[0]
            fake_in, cond_in = fake_videos, cond
            if aug or geo:
                # the generator step reuses fake_s / fake_d, so its gradient passes through the transform (autograd sums the two
                # discriminators' gradients before the one backward launch of each stage); the context frames take the FAKE
                # clips' rows
                fake_in = self._d_view(fake_videos, mat_fake, tab_fake)
                if cond is not None:
                    cond_in = self._d_view(cond, mat_fake, tab_fake)
            fake_s = sample_k_frames(fake_in, T, k, ids_fake)
            # ---------------- D_s
            if early:
                cur.wait_stream(self._aux)
                for t_ in (ds_loss_real, dt_loss_real, real_d):
                    t_.record_stream(cur)
            else:
                ds_loss_real = self._site_loss(self.D_s(real_s, real_labels), True, 0)
            ds_loss_fake = self._site_loss(self.D_s(fake_s.detach(), z_class), False, 1)
            self.reset_grad()
            (ds_loss_real + ds_loss_fake).backward()
            Fn.join_side()
            ex.start("Ds", self.ds_optimizer.grad)
            # ---------------- D_t (its forward/backward overlaps the D_s gradient exchange)
            fake_d = vid_downsample(fake_in) if cond is None else vid_downsample_cat(cond_in, fake_in)
            if not early:
                real_d = vid_downsample(real_in)
                dt_loss_real = self._site_loss(self.D_t(real_d, real_labels), True, 2)
            dt_loss_fake = self._site_loss(self.D_t(fake_d.detach(), z_class), False, 3)
            ex.finish("Ds")
            self.ds_optimizer.step()
            self.ds_lr_scher.step((ds_loss_real + ds_loss_fake) if self._plateau else None)
            self.dt_optimizer.zero_grad()
            (dt_loss_real + dt_loss_fake).backward()
            Fn.join_side()
            ex.start("Dt", self.dt_optimizer.grad)
            self._end_d_iteration()
            last = _ == self.d_iters - 1
            if not last:
                ex.finish("Dt")
                self.dt_optimizer.step()
                self.dt_lr_scher.step((dt_loss_real + dt_loss_fake) if self._plateau else None)
        # ---------------- G, through the updated discriminators, weights of D held constant.  The D_t gradient exchange
        # of the last D iteration overlaps the D_s forward (D_s is already updated; D_t's update waits for the exchange)
        self._freeze_d(True)
        g_s_loss = self._site_loss(self.D_s(fake_s, z_class), True, 4)
        ex.finish("Dt")
        self.dt_optimizer.step()
        self.dt_lr_scher.step((dt_loss_real + dt_loss_fake) if self._plateau else None)
        g_t_loss = self._site_loss(self.D_t(fake_d, z_class), True, 5)
        self._freeze_d(False)
        self.g_optimizer.zero_grad()
        if ex.active:
            # bucketed exchange: the tail of the flat gradient buffer (last modules) is final first
            self._g_hi = self.g_optimizer.grad.numel()

            def on_ready(first_done, self=self, ex=ex):
                lo = self._g_bounds[first_done]
                # the bucket's weight gradients were queued on the side stream: the EXCHANGE stream waits for them -- the
                # step's chain is not fenced (round 6: joining the side stream here serialised the backward pass behind every
                # queued weight-gradient launch three times per step, bench.py --force-exchange)
                ex.start_range("G", self.g_optimizer.grad, lo, self._g_hi, after=(Fn.side_stream_if_any(),))
                self._g_hi = min(self._g_hi, lo)
            self.G.grad_ready_hook = on_ready
        (g_s_loss + g_t_loss).backward()
        Fn.join_side()
        if ex.active:
            self.G.grad_ready_hook = None
            ex.start_range("G", self.g_optimizer.grad, 0, self._g_hi)
        ex.finish("G")
        self.g_optimizer.step()
        self.g_lr_scher.step((g_s_loss + g_t_loss) if self._plateau else None)
        if aug or geo:
            self._aug_adapt()
        if getattr(self, "sv_log", 0):
            self._sv_steps += 1
            if self._sv_steps % self.sv_log == 0:
                self._sv_log_row()
        return ds_loss_real, ds_loss_fake, dt_loss_real, dt_loss_fake, g_s_loss, g_t_loss

    # ---- trainer.py:189-343 (loop; logging reduced to a print)
    def _new_epoch(self):
        """-> iterator over the loader for the next epoch.  A rank-sharded loader (data.make_loader: DistributedSampler) shuffles
        with seed + epoch: without set_epoch every epoch would repeat the same order and the same rank split."""
        if hasattr(self.data_loader, "set_epoch"):
            self.data_loader.set_epoch(self._epoch)
        elif hasattr(getattr(self.data_loader, "sampler", None), "set_epoch"):
            self.data_loader.sampler.set_epoch(self._epoch)
        self._epoch += 1
        return iter(self.data_loader)

    def train(self):
        steps_per_epoch = len(self.data_loader)
        total_step = self.total_epoch * steps_per_epoch
        start = (self.pretrained_model + 1) if self.pretrained_model else 1
        self._epoch = (start - 1) // max(1, steps_per_epoch)       # a resumed run continues with the epoch it stopped in
        data_iter = None
        state_file = self._resume_file()
        if state_file is not None:
            # exact resume: weights, Adam, schedules, random streams and -- where the loader keeps one -- the position inside the
            # epoch are those of the saved step; the loop goes on with the step after it
            self.load_state(state_file)
            start = self._resumed_step + 1
            if self._loader_resumed:
                data_iter = iter(self.data_loader)                  # the saved epoch, continued: no new order, no draw
            else:
                self._epoch = (start - 1) // max(1, steps_per_epoch)       # a loader without state: its epoch starts over
        if data_iter is None:
            data_iter = self._new_epoch()
        state_save_step = getattr(self, "state_save_step", 0)
        self.D_s.train(); self.D_t.train(); self.G.train()
        t0 = time.time()
        # sample sheets: every sample_step steps, or every sample_epoch epochs (trainer.py:186); 0 = never, nothing is set up
        sample_step = getattr(self, "sample_step", 0) or int(getattr(self, "sample_epoch", 0) * steps_per_epoch)
        try:
            for step in range(start, total_step + 1):
                try:
                    real_videos, real_labels = next(data_iter)
                except StopIteration:
                    data_iter = self._new_epoch()
                    real_videos, real_labels = next(data_iter)
                losses = self.train_step(real_videos, real_labels)
                if state_save_step and step % state_save_step == 0:
                    self.save_state(step)
                if self.log_epoch and step % (self.log_epoch * steps_per_epoch) == 0:
                    vals = [float(v.detach()) for v in losses]
                    line = ("Step: [%d/%d], time: %.1fs, ds_loss: %.4f, dt_loss: %.4f, g_s_loss: %.4f, g_t_loss: %.4f, lr: %.2e"
                            % (step, total_step, time.time() - t0, vals[0] + vals[1], vals[2] + vals[3], vals[4], vals[5],
                               self.g_lr_scher.get_lr()[0]))
                    for tag, rep in (self.guard_report() or {}).items():
                        if rep is not None:
                            line += ", %s |g|: %.3e skipped: %d" % (tag, rep["norm"], rep["skipped"])
                    rep = self.d_stats() if getattr(self, "_adv_stats", None) is not None else None
                    for tag in ("Ds", "Dt") if rep else ():
                        line += ", %s r_t: %.3f lecam: %.3e/%.3e" % (tag, rep[tag]["r_t"], rep[tag]["lecam_real"],
                                                                     rep[tag]["lecam_fake"])
                    if getattr(self, "d_aug", ()) or getattr(self, "d_aug_geom", ()):
                        line += ", d_aug p: %.4f" % self.d_aug_p
                    print(line)
                if sample_step and step % sample_step == 0:
                    self.save_samples(step)
                if self.model_save_epoch and step % (self.model_save_epoch * steps_per_epoch) == 0:
                    self.save_models(step)
        except BaseException:
            self.close_sheets(quiet=True)          # the loop's exception is the one to report
            self.close_state(quiet=True)
            raise
        self.close_sheets()
        self.close_state()

    # ---- exact resume: the full training state (checkpoint.py; DESIGN section 8, "what a step leaves for the next")
    def _nets(self):
        return (("G", self.G), ("Ds", self.D_s), ("Dt", self.D_t))

    def _schedulers(self):
        return (("G", self.g_lr_scher), ("Ds", self.ds_lr_scher), ("Dt", self.dt_lr_scher))

    def fingerprint(self):
        """The fields that decide shapes and arithmetic (checkpoint.FINGERPRINT): a state continues only a Trainer that agrees
        in all of them."""
        c = self.config
        return {"g_chn": int(self.g_chn), "ds_chn": int(self.ds_chn), "dt_chn": int(self.dt_chn), "n_frames": int(self.n_frames),
                "n_cond": int(self.n_cond), "n_class": int(self.n_class), "z_dim": int(self.z_dim),
                "latent_dim": int(self.latent_dim), "g_self_attn": bool(getattr(c, "g_self_attn", False)),
                "g_sep_attn": bool(getattr(c, "g_sep_attn", False)), "compute_dtype": str(self.compute_dtype),
                "adv_loss": str(self.adv_loss), "d_iters": int(self.d_iters), "k_sample": int(self.k_sample),
                "batch_size": int(self.batch_size), "world_size": int(D.world_size()), "dp_mode": str(self.dp_mode)}

    def _resume_file(self):
        """config.resume -> the state file to continue from, or None (unset, or "latest" with no complete file yet)."""
        resume = getattr(self, "resume", None)
        if not resume:
            return None
        if resume != "latest":
            return resume
        from .checkpoint import latest_state
        found = latest_state(self.model_save_path)
        return None if found is None else found[1]

    def _host_state(self):
        """This process's own host-side state: its random streams (torch's default generator, Python's `random`, numpy's
        global state, noise_gen) and its loader's position.  The device generator is not in it: nothing in the package draws
        from it."""
        from .checkpoint import host_rng_state
        loader = self.data_loader.state_dict() if hasattr(self.data_loader, "state_dict") else None
        out = {"rng": host_rng_state((("noise_gen", self.noise_gen),)), "loader": loader}
        if getattr(self, "d_aug", ()) or getattr(self, "d_aug_geom", ()):
            # the augmentation's own state: the current p, the tables' generator, steps and adjustments made so far
            out["aug"] = {"p": float(self.d_aug_p), "generator": self._aug_gen.get_state().clone(),
                          "steps": int(self._aug_steps), "adjustments": int(self._aug_adjustments)}
        return out

    def save_state(self, step, wait=False):
        """Write everything step `step` leaves for step + 1 as `{step}_state.pt` under config.model_save_path/version: the
        three networks' state_dict()s (the trained weights as the optimizers' flat buffers, every other entry by name), the three
        FlatAdam states (m, v, the weight average, t, lr, the guard's counters and log), the three schedules, step and epoch,
        the loader's position and the host random streams.  Call it between two train_step() calls, on the stream they are
        called on.  `load_state` of that file into a Trainer of the same configuration continues the run bit for bit.
        wait=False: the state is copied device-to-device into a staging slab on the current stream, the host-side state is
        captured at the same moment, and this call returns; a copy stream takes the slab to pinned memory and a worker thread
        writes the file (checkpoint.StateWriter, where the memory this costs is stated) -- the calling thread does not wait
        for the device, and the training step may go on at once.  One snapshot is outstanding at most: a second save_state()
        first waits for the first file.  wait=True returns when the file is complete.  A file under its final name is complete
        (written as `.tmp`, fsync'ed, renamed); config.state_keep = n keeps the n newest states.  An exception of the worker is
        raised by the next save_state() or by close_state().
        Data parallel: rank 0 writes the file above; every rank writes its own random streams and loader position as
        `{step}_state.rank{r}.pt`, synchronously (a few kB)."""
        from . import checkpoint as C
        folder, step = self.model_save_path, int(step)
        world, keep = D.world_size(), getattr(self, "state_keep", 2)
        os.makedirs(folder, exist_ok=True)
        own = self._host_state()
        if world > 1:
            C.atomic_save({"format_version": C.FORMAT_VERSION, "step": step, "rank": self.rank, "host": own},
                          C.state_path(folder, step, self.rank))
            if self.rank != 0:
                return
        host = {"step": step, "epoch": int(getattr(self, "_epoch", 0)), "opt": {}, "sched": {}, "rng": own["rng"],
                "loader": own["loader"], "frame_gen": None if self.frame_gen is None else self.frame_gen.get_state().clone()}
        if "aug" in own:
            host["aug"] = own["aug"]
        items, slabs = [], {}
        copy_of = lambda t: (lambda dst: dst.copy_(t))
        for tag, net in self._nets():
            trained = {k for k, p in net.named_parameters() if p.requires_grad}
            for k, v in net.state_dict().items():
                if k not in trained:                    # the trained weights are views of the optimizer's `flat`
                    items.append((f"net.{tag}.{k}", v.dtype, tuple(v.shape), copy_of(v)))
        for (tag, opt), (_, sched) in zip(self._optimizers(), self._schedulers()):
            slabs[tag] = (["flat", "m", "v"] + (["ema"] if opt.ema is not None else []), opt.flat.numel())
            items.append((f"opt.{tag}.slab", torch.float32, (opt.snapshot_numel(),), opt.snapshot_into))
            for k in ("guard_state", "guard_ring", "ortho_penalty"):
                t = getattr(opt, k)
                if t is not None:
                    items.append((f"opt.{tag}.{k}", t.dtype, tuple(t.shape), copy_of(t)))
            host["opt"][tag] = dict(opt.settings(), t=int(opt.t), lr=float(opt.param_groups[0]["lr"]), numel=int(opt.flat.numel()))
            host["sched"][tag] = sched.state_dict()
        if getattr(self, "_anchors", None) is not None:       # LeCam: both slots of each discriminator's anchors and the count
            for net, tag in enumerate(("Ds", "Dt")):
                items.append((f"lecam.{tag}", torch.float32, (2, 2), copy_of(self._anchors[:, net])))
            host["lecam_it"] = int(self._lecam_it)
        fingerprint = self.fingerprint()

        def make_file(tensors):
            for tag, (parts, n) in slabs.items():
                slab = tensors.pop(f"opt.{tag}.slab")
                for i, k in enumerate(parts):
                    tensors[f"opt.{tag}.{k}"] = slab[i * n:(i + 1) * n]
            return {"format_version": C.FORMAT_VERSION, "step": step, "fingerprint": fingerprint, "tensors": tensors, "host": host}

        if self._state_writer is None:
            self._state_writer = C.StateWriter()
        self._state_writer.submit(C.state_path(folder, step), items, make_file, device=self.device,
                                  after=lambda: C.prune_states(folder, keep), wait=wait)

    def close_state(self, quiet=False):
        """Wait for the state file that is being written and end the writer's thread (a later save_state() starts a new one);
        its buffers are given back.  An exception the file hit is raised here, unless quiet."""
        w, self._state_writer = getattr(self, "_state_writer", None), None
        if w is not None:
            try:
                w.close()
            except Exception:
                if not quiet:
                    raise

    def load_state(self, path):
        """Continue from the file save_state() wrote: copies every tensor into the existing buffers (no parameter is rebound),
        sets the optimizers' t / lr, the schedules, step and epoch, the loader's position (when the loader has
        load_state_dict()) and the host random streams.  Read with weights_only=True.  ValueError naming the field on an
        unknown format_version, on the first fingerprint field that differs, and on a tensor that is missing or of another
        shape.  In a data-parallel run every rank reads this file and its own `{step}_state.rank{r}.pt` next to it.  -> list of
        warning strings (settings that only steer future steps and differ from the file's; the constructor's hold)."""
        from . import checkpoint as C
        sd = C.load_file(path)
        C.check_fingerprint(sd["fingerprint"], self.fingerprint())
        tensors, host, step = sd["tensors"], sd["host"], int(sd["step"])
        own = host
        if D.world_size() > 1:
            rank_file = C.state_path(os.path.dirname(path), step, self.rank)
            own = C.load_file(rank_file)["host"]
        for tag, net in self._nets():
            trained = {k for k, p in net.named_parameters() if p.requires_grad}
            for k, v in net.state_dict().items():
                if k in trained:
                    continue
                src = tensors.get(f"net.{tag}.{k}")
                if src is None or tuple(src.shape) != tuple(v.shape) or src.dtype != v.dtype:
                    raise ValueError(f"net.{tag}.{k}: the state holds {None if src is None else (src.dtype, tuple(src.shape))}, "
                                     f"the network {(v.dtype, tuple(v.shape))}")
                v.copy_(src)
        notes = []
        for (tag, opt), (_, sched) in zip(self._optimizers(), self._schedulers()):
            osd = dict(host["opt"][tag])
            for k in ("flat", "m", "v", "ema", "guard_state", "guard_ring", "ortho_penalty"):
                osd[k] = tensors.get(f"opt.{tag}.{k}")
            if osd["flat"] is None or osd["m"] is None or osd["v"] is None:
                raise ValueError(f"opt.{tag}: the state holds no flat / m / v for this optimizer")
            notes += [f"{tag}: {n}" for n in opt.load_state_dict(osd)]
            sched.load_state_dict(host["sched"][tag])
        if getattr(self, "_anchors", None) is not None:
            saved = [tensors.get(f"lecam.{tag}") for tag in ("Ds", "Dt")]
            if any(t is None or tuple(t.shape) != (2, 2) for t in saved) or "lecam_it" not in host:
                self._anchors.zero_()
                self._lecam_it = 0
                notes.append("lecam: the state holds no anchors (it was written with lecam off): they start afresh")
            else:
                for net, t in enumerate(saved):
                    self._anchors[:, net].copy_(t)
                self._lecam_it = int(host["lecam_it"])
        if getattr(self, "d_aug", ()) or getattr(self, "d_aug_geom", ()):
            saved = own.get("aug")
            if saved is None:                   # the LeCam anchors' rule: the constructor's p, a fresh generator, and a note
                self.d_aug_p = float(getattr(self.config, "d_aug_p", 1.0))
                self._aug_gen = self._new_aug_gen()
                self._aug_steps = self._aug_adjustments = 0
                notes.append("d_aug: the state holds no augmentation state (it was written with d_aug off): p and the tables' "
                             "generator start afresh")
            else:
                self.d_aug_p = float(saved["p"])
                self._aug_gen.set_state(saved["generator"])
                self._aug_steps, self._aug_adjustments = int(saved["steps"]), int(saved["adjustments"])
        self._epoch, self._resumed_step = int(host["epoch"]), step
        self._loader_resumed = own.get("loader") is not None and hasattr(self.data_loader, "load_state_dict")
        if self._loader_resumed:
            self.data_loader.load_state_dict(own["loader"])
        if self.frame_gen is not None and host.get("frame_gen") is not None:
            self.frame_gen.set_state(host["frame_gen"])
        C.set_host_rng_state(own["rng"], (("noise_gen", self.noise_gen),))
        return notes

    # ---- trainer.py:195-197, 323-334, 389-391: sample sheets (sheets.py)
    def fixed_inputs(self):
        """-> (fixed_z [n_class * test_batch_size, z_dim], fixed_label [n_class * test_batch_size]) on the device: the values of
        trainer.py:195-197, test_batch_size clips per class in class order.  z comes from a private generator seeded with
        config.sample_seed (the default generator and noise_gen are not touched); drawn once, uploaded once."""
        if self._fixed is None:
            gen = torch.Generator().manual_seed(self.sample_seed)
            z = torch.randn(self.test_batch_size * self.n_class, self.z_dim, generator=gen)
            label = torch.tensor([i for i in range(self.n_class) for j in range(self.test_batch_size)])
            self._fixed = (to_device_async(z, self.device), to_device_async(label, self.device))
        return self._fixed

    @property
    def sheet_writer(self):
        """The sheets.SheetWriter the save_* calls submit to (made at first use; `sheet_writer.flush()` waits for the files)."""
        if self._sheets is None:
            from .sheets import SheetWriter
            self._sheets = SheetWriter(max_pending=2)
        return self._sheets

    def close_sheets(self, quiet=False):
        """Wait for the pending files and end the writer's thread (a later save_* call starts a new one).  An exception a file
        hit is raised here, unless quiet."""
        w, self._sheets = getattr(self, "_sheets", None), None
        if w is not None:
            try:
                w.close()
            except Exception:
                if not quiet:
                    raise

    def _is_writer(self):
        return D.world_size() == 1 or torch.distributed.get_rank() == 0

    @torch.no_grad()
    def save_samples(self, step, fixed_z=None, fixed_label=None, *, chunk=None):
        """trainer.py:323-334: eval-mode G on the fixed noise, written as sheets under config.sample_path/version.  The clips are
        generated at most `chunk` at a time (default batch_size), every chunk from the same generator state, and one launch per
        chunk (sheets.make_sheets on the raw [-1, 1] output: denorm, 8-bit, tiling, RGB interleave) writes straight into the
        buffer of the whole job, which the writer thread copies out, compresses and writes -- this call waits for none of it.
        config.sample_layout "frames": `Class_%d_No.%d_Step_%d.png` per clip, its n_frames frames in rows of 8 (the reference's
        files, with the extension it left out).  "clips": `Step_%d.apng`, one animation frame per time step showing every clip, a
        row per class, config.sample_fps frames a second.  "both": both.
        config.sample_use_ema computes with the averaged weights (ema_weights() entered once, config.ema_standing_stats passes).
        Leaves no trace: weights, spectral-norm u / v, batch-norm statistics and counters are bit-equal before and after (unlike
        the reference and sample(), whose u / v advance), and no random generator of the run is touched.  In a data-parallel run
        every rank runs the passes and rank 0 writes."""
        from .sheets import make_sheets
        if self.n_cond:
            raise RuntimeError("a frame-conditional generator (n_cond > 0) continues clips: use save_predictions(step, clips, labels)")
        if (fixed_z is None) != (fixed_label is None):
            raise ValueError("give both fixed_z and fixed_label, or neither (fixed_inputs())")
        if fixed_z is None:
            z, label = self.fixed_inputs()              # on the device already, in range by construction: no host sync
            numbering = [(i, j) for i in range(self.n_class) for j in range(self.test_batch_size)]
        else:
            z, label = to_device_async(fixed_z, self.device), to_device_async(self._check_labels(fixed_label), self.device)
            numbering = self._class_and_number(fixed_label)
        n = z.shape[0]
        if n < 1 or label.shape[0] != n:
            raise ValueError(f"fixed_z {tuple(z.shape)} and fixed_label {tuple(label.shape)} must hold the same number of clips")
        chunk = int(self.batch_size if chunk is None else chunk)
        if chunk < 1:
            raise ValueError(f"chunk={chunk}")
        per_class = self.test_batch_size if n == self.n_class * self.test_batch_size else min(n, 8)
        do_frames, do_clips = self.sample_layout in ("frames", "both"), self.sample_layout in ("clips", "both")
        by_clip = by_step = None
        with self._sampling_weights(self.sample_use_ema, None):
            frozen = self._g_frozen_tensors()
            saved = [t.clone() for t in frozen]
            self.G.eval()
            try:
                for lo in range(0, n, chunk):
                    raw = self.G(z[lo:lo + chunk], label[lo:lo + chunk])          # [b, T, 3, H, W] in [-1, 1]
                    for t, old in zip(frozen, saved):
                        t.copy_(old)
                    if do_frames:
                        if by_clip is None:
                            by_clip = torch.empty((n,) + self._sheet_dims(raw.shape[1], raw, 8), dtype=torch.uint8, device=self.device)
                        make_sheets(raw, layout="frames", row_prefix=True, out=by_clip[lo:lo + raw.shape[0]])
                    if do_clips:
                        if by_step is None:
                            by_step = torch.empty((raw.shape[1],) + self._sheet_dims(n, raw, per_class), dtype=torch.uint8,
                                                  device=self.device)
                        make_sheets(raw, layout="clips", nrow=per_class, row_prefix=True, out=by_step, first_slot=lo, total_slots=n,
                                    fill=lo == 0)
            finally:
                self.G.train()
                for t, old in zip(frozen, saved):
                    t.copy_(old)
        if self._is_writer():
            os.makedirs(self.sample_path, exist_ok=True)
            if do_frames:
                names = [os.path.join(self.sample_path, "Class_%d_No.%d_Step_%d.png" % (c, j, step)) for c, j in numbering]
                self.sheet_writer.submit("png", names, by_clip)
            if do_clips:
                self.sheet_writer.submit("apng", os.path.join(self.sample_path, "Step_%d.apng" % step), by_step,
                                         fps=self.sample_fps, loops=0)

    @staticmethod
    def _sheet_dims(n_tiles, frames, nrow):
        from .sheets import sheet_shape
        Hs, Ws = sheet_shape(n_tiles, frames.shape[-2], frames.shape[-1], nrow)
        return Hs, 1 + 3 * Ws

    @staticmethod
    def _class_and_number(labels):
        """(class, running number within the class) per clip, in clip order: trainer.py:327-332's (i, j) for its fixed labels."""
        seen, out = {}, []
        for c in labels.tolist():
            out.append((c, seen.get(c, 0)))
            seen[c] = seen.get(c, 0) + 1
        return out

    @torch.no_grad()
    def save_predictions(self, step, clips, labels, *, n_samples=1, horizon=None, seed=0):
        """Comparison sheets of a frame-conditional generator (n_cond = K > 0): clips [B, 3, K + horizon, H, W] in [-1, 1] as the
        loader delivers them (horizon defaults to n_frames; longer ones are rolled out like rollout()), labels [B] ->
        `Pred_%d_Step_%d.png` per clip.  Its first row of K + horizon slots holds the real [context | future] frames, row 1 + s
        the context followed by sampled future s = rollout(cond, labels, horizon, z=z_s), the z of evaluate_prediction(seed=seed)
        (a private generator).  Every row is written by launches of its own from the views (sheets.make_sheets(first_slot=...)):
        no concatenated copy.  Leaves no trace, like evaluate_prediction()."""
        from .sheets import make_sheets
        K_ = self.n_cond
        horizon = self.n_frames if horizon is None else int(horizon)
        self._rollout_args("save_predictions", clips, horizon, (2, K_ + horizon))
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError(f"n_samples={n_samples}")
        B, L_ = clips.shape[0], K_ + horizon
        gen = torch.Generator().manual_seed(int(seed))
        clips = to_device_async(clips, self.device).to(torch.float32)
        frames = clips.permute(0, 2, 1, 3, 4)                          # [B, K + horizon, 3, H, W], a view
        ctx_view, cond = frames[:, :K_], frames[:, :K_].contiguous()
        labels_d = to_device_async(self._check_labels(labels), self.device)
        zs = to_device_async(torch.stack([torch.randn(B, self.z_dim, generator=gen) for _ in range(n_samples)]), self.device)
        total = (1 + n_samples) * L_
        out = torch.empty((B,) + self._sheet_dims(total, frames, L_), dtype=torch.uint8, device=self.device)
        make_sheets(frames, nrow=L_, row_prefix=True, out=out, total_slots=total)                  # row 0, borders, every other slot
        frozen = self._g_frozen_tensors()
        saved = [t.clone() for t in frozen]
        self.G.eval()
        try:
            for s in range(n_samples):
                z = zs[s]
                raw = self._rollout_raw(cond, labels_d, horizon, lambda: z)
                for t, old in zip(frozen, saved):
                    t.copy_(old)
                make_sheets(ctx_view, nrow=L_, row_prefix=True, out=out, first_slot=(1 + s) * L_, total_slots=total, fill=False)
                make_sheets(raw, nrow=L_, row_prefix=True, out=out, first_slot=(1 + s) * L_ + K_, total_slots=total, fill=False)
        finally:
            self.G.train()
            for t, old in zip(frozen, saved):
                t.copy_(old)
        if self._is_writer():
            os.makedirs(self.sample_path, exist_ok=True)
            self.sheet_writer.submit("png", [os.path.join(self.sample_path, "Pred_%d_Step_%d.png" % (b, step)) for b in range(B)], out)

    @torch.no_grad()
    def save_real(self, real_videos):
        """trainer.py:389-391: the loader's clips [B, 3, T, H, W] in [-1, 1] -> `real_%d.png` per clip, the sheet save_samples
        writes for a generated one (read through the clip's strides: no permuted copy)."""
        from .sheets import make_sheets
        if real_videos.dim() != 5 or real_videos.shape[1] != 3:
            raise ValueError(f"real_videos {tuple(real_videos.shape)} must be [B, 3, T, H, W]")
        clips = to_device_async(real_videos, self.device).to(torch.float32)
        out = make_sheets(clips.permute(0, 2, 1, 3, 4), row_prefix=True)
        if self._is_writer():
            os.makedirs(self.sample_path, exist_ok=True)
            self.sheet_writer.submit("png", [os.path.join(self.sample_path, "real_%d.png" % b) for b in range(out.shape[0])], out)

    # ---- the averaged generator weights
    def _ema_on(self):
        return bool(getattr(getattr(self, "g_optimizer", None), "ema_decay", 0.0))

    def _g_frozen_tensors(self):
        """Every tensor of G that Adam does not own: spectral-norm u / v, batch-norm running statistics and counters."""
        return [p.data for p in self.G.parameters() if not p.requires_grad] + list(self.G.buffers())

    def standing_draws(self, generator, batch):
        """z [batch, z_dim] and labels [batch] of ONE standing-statistics pass, in the order the passes draw them."""
        z = torch.randn(batch, self.z_dim, generator=generator)
        return z, torch.randint(0, self.n_class, (batch,), generator=generator)

    @contextlib.contextmanager
    def ema_weights(self, standing_stats=0, cond=None, labels=None):
        """Inside the block `self.G` computes with the averaged weights: the average and the live weights are exchanged in
        place (dvd_swap_f32) on entry and exchanged back on exit, and every tensor of G that is not a trained weight (spectral-
        norm u / v, batch-norm running statistics and counters) is put back as it was -- training state after the block is
        bit-equal to before it.  Before the first optimizer step the average IS the weights and nothing is exchanged.
        Not re-entrant: a second block inside the first would exchange the live weights back in, so it raises.
        standing_stats = N > 0: on entry, after the exchange, the running statistics are re-estimated for the averaged weights
        by N train-mode forward passes without gradients, pass i with batch-norm momentum 1 / i (a cumulative average from
        scratch), on z / labels from a private generator seeded with config.ema_stats_seed (the default generator is not
        touched).  A frame-conditional generator runs them on the caller's `cond` / `labels`."""
        if not self._ema_on():
            raise RuntimeError("no weight average is configured (config.ema_decay = 0)")
        if getattr(self, "_ema_block", False):
            raise RuntimeError("ema_weights() is already active: the block does not nest (save_models and sample / predict with "
                               "use_ema=True enter it themselves)")
        from .sn_layers import ConditionalNorm
        opt, G = self.g_optimizer, self.G
        n_pass = int(standing_stats or 0)
        if n_pass and self.n_cond and (cond is None or labels is None):
            raise ValueError("standing statistics of a frame-conditional generator need the caller's `cond` and `labels`")
        frozen = self._g_frozen_tensors()
        saved = [t.clone() for t in frozen]
        norms = [m for m in G.modules() if isinstance(m, ConditionalNorm)]
        momenta, was_training = [m.momentum for m in norms], G.training
        swapped = opt.ema is not None
        self._ema_block = True
        if swapped:
            K.swap_(opt.flat, opt.ema)
        try:
            if n_pass:
                gen = torch.Generator().manual_seed(self.ema_stats_seed)
                B = cond.shape[0] if self.n_cond else self.batch_size
                G.train()
                for m in norms:                    # from scratch: nothing of the live statistics (a NaN included) survives
                    m.bn.num_batches_tracked.zero_()
                    m.bn.running_mean.zero_()
                    m.bn.running_var.fill_(1.0)
                with torch.no_grad():
                    for i in range(1, n_pass + 1):
                        for m in norms:
                            m.momentum = 1.0 / i
                        z, y = self.standing_draws(gen, B)
                        if self.n_cond:
                            G(z.to(self.device), self._check_labels(labels).to(self.device), cond=cond.to(self.device, torch.float32))
                        else:
                            G(z.to(self.device), y.to(self.device))
                for m, mom in zip(norms, momenta):
                    m.momentum = mom
                G.train(was_training)
            yield self.G
        finally:
            for m, mom in zip(norms, momenta):
                m.momentum = mom
            G.train(was_training)
            if swapped:
                K.swap_(opt.flat, opt.ema)
            for t, old in zip(frozen, saved):
                t.copy_(old)
            self._ema_block = False

    def _sampling_weights(self, use_ema, standing_stats, cond=None, labels=None):
        if not use_ema:
            if standing_stats:
                raise ValueError("standing_stats re-estimates the statistics of the averaged weights: it needs use_ema=True")
            return contextlib.nullcontext()
        if not self._ema_on():
            raise RuntimeError("use_ema=True, but no weight average is configured (config.ema_decay = 0)")
        n = self.ema_standing_stats if standing_stats is None else int(standing_stats)
        return self.ema_weights(n, cond=cond, labels=labels)

    def _draw_z(self, batch, truncation):
        if truncation is None:
            return torch.randn(batch, self.z_dim, generator=self.noise_gen)
        return truncated_z(batch, self.z_dim, truncation, generator=self.noise_gen)

    # ---- trainer.py:323-334: the sampling path (eval-mode G on fixed z / labels, BN running statistics); the image files are
    # save_samples() above (tensorboard stays out)
    @torch.no_grad()
    def sample(self, fixed_z, fixed_label, *, use_ema=False, standing_stats=None, truncation=None):
        """-> denorm(G(fixed_z, fixed_label)) [B, T, 3, H, W] in [0, 1]; G is put back in train mode, like the reference.
        Note quirk 2: the spectral-norm u/v of G advance in eval mode as well.
        use_ema: compute with the averaged weights (ema_weights(); the training state is left untouched, u / v included);
        standing_stats: passes that re-estimate the batch-norm statistics for them (None = config.ema_standing_stats).
        fixed_z = None draws z here, truncation = tau from N(0, 1) truncated to [-tau, tau] (helpers.truncated_z)."""
        if self.n_cond:
            raise RuntimeError("a frame-conditional generator (n_cond > 0) continues clips: use Trainer.predict(cond, labels)")
        if fixed_z is None:
            fixed_z = self._draw_z(fixed_label.shape[0], truncation)
        elif truncation is not None:
            raise ValueError("truncation applies to z drawn here: pass fixed_z=None, or truncate the z you pass")
        with self._sampling_weights(use_ema, standing_stats):
            self.G.eval()
            try:
                fake = self.G(fixed_z.to(self.device), fixed_label.to(self.device))
            finally:
                self.G.train()
        return denorm(fake)

    @torch.no_grad()
    def predict(self, cond, labels, z=None, *, use_ema=False, standing_stats=None, truncation=None):
        """Frame-conditional prediction (n_cond = K > 0): cond [B, K, 3, H, W] context frames in [-1, 1] (the generator's output
        layout, so denormalised predictions come back in as 2 p - 1), labels [B] -> denorm(G(z, labels, cond=cond)), the next
        n_frames frames [B, T, 3, H, W] in [0, 1].  z [B, z_dim] defaults to a fresh draw (truncated to [-truncation,
        truncation] when that is given).  Eval / train mode, use_ema and standing_stats as in sample(); the standing-statistics
        passes run on this call's cond / labels."""
        if not self.n_cond:
            raise RuntimeError("predict() needs a frame-conditional Trainer (config.n_cond > 0); use sample()")
        B = cond.shape[0]
        if z is None:
            z = self._draw_z(B, truncation)
        elif truncation is not None:
            raise ValueError("truncation applies to z drawn here: pass z=None, or truncate the z you pass")
        with self._sampling_weights(use_ema, standing_stats, cond, labels):
            self.G.eval()
            try:
                fake = self.G(z.to(self.device), self._check_labels(labels).to(self.device), cond=cond.to(self.device, torch.float32))
            finally:
                self.G.train()
        return denorm(fake)

    # ---- autoregressive rollouts and the prediction metrics (no counterpart in the reference)
    def _rollout_raw(self, cond, labels, horizon, draw_z):
        """The chunks of a rollout, RAW ([-1, 1], as the generator wrote them): [B, horizon, 3, H, W].  cond / labels on the
        device; draw_z() -> the z of the next chunk (a device tensor is used as it is, a host tensor goes up without stalling the
        host); G in eval mode and the weights chosen by the caller."""
        K_, T = self.n_cond, self.n_frames
        chunks, ctx = [], cond
        for done in range(0, horizon, T):
            fake = self.G(to_device_async(draw_z(), self.device), labels, cond=ctx)
            chunks.append(fake)
            if done + T < horizon:
                # the last K frames of [context | everything generated so far], untouched: no denorm and back
                ctx = (fake[:, -K_:] if T >= K_ else torch.cat([ctx, fake], 1)[:, -K_:]).contiguous()
        out = chunks[0] if len(chunks) == 1 else torch.cat(chunks, 1)
        return out if out.shape[1] == horizon else out[:, :horizon].contiguous()

    def _rollout_args(self, what, cond, horizon, n_frames_ctx):
        if not self.n_cond:
            raise RuntimeError(f"{what}() needs a frame-conditional Trainer (config.n_cond > 0); use sample()")
        if int(horizon) < 1:
            raise ValueError(f"horizon={horizon}")
        if cond.dim() != 5 or cond.shape[n_frames_ctx[0]] != n_frames_ctx[1]:
            raise ValueError(f"{what}(): unexpected clip shape {tuple(cond.shape)} for n_cond={self.n_cond}, horizon={horizon}")

    @torch.no_grad()
    def rollout(self, cond, labels, horizon, z=None, *, use_ema=False, standing_stats=None, truncation=None):
        """Autoregressive prediction past the training length: cond [B, K, 3, H, W] context frames in [-1, 1], labels [B] ->
        [B, horizon, 3, H, W] in [0, 1].  n_frames are predicted at a time; every further chunk is conditioned on the last K
        frames of [context | everything generated so far] exactly as the generator produced them (raw [-1, 1] values), and the
        last chunk is cut to `horizon` -- so horizon == n_frames is predict() bit for bit.  z [B, z_dim] serves every chunk when
        given; otherwise each chunk draws its own (truncated to [-truncation, truncation] when that is given).  use_ema /
        standing_stats as in predict(): the ema_weights() block is entered ONCE around the whole rollout, the standing-statistics
        passes run once, on the caller's cond / labels.
        Unlike predict(), which advances the generator's spectral-norm u / v even in eval mode (quirk 2), a rollout leaves NO trace:
        u / v advance from chunk to chunk inside it and are put back at the end, so weights, u / v, batch-norm statistics and
        counters are bit-equal before and after and a rollout in the middle of training does not move the run."""
        self._rollout_args("rollout", cond, horizon, (1, self.n_cond))
        B = cond.shape[0]
        if z is not None and truncation is not None:
            raise ValueError("truncation applies to z drawn here: pass z=None, or truncate the z you pass")
        if z is not None:
            z = to_device_async(z, self.device)                 # one upload serves every chunk
        draw = (lambda: z) if z is not None else (lambda: self._draw_z(B, truncation))
        with self._sampling_weights(use_ema, standing_stats, cond, labels):
            frozen = self._g_frozen_tensors()
            saved = [t.clone() for t in frozen]
            self.G.eval()
            try:
                raw = self._rollout_raw(cond.to(self.device, torch.float32),
                                        to_device_async(self._check_labels(labels), self.device), int(horizon), draw)
            finally:
                self.G.train()
                for t, old in zip(frozen, saved):
                    t.copy_(old)
        return denorm(raw)

    @torch.no_grad()
    def evaluate_prediction(self, clips, labels, *, horizon=None, n_samples=1, seed=0, use_ema=False, standing_stats=None,
                            truncation=None, quantize=True):
        """PSNR / SSIM of predicted futures against the held-out frames of real clips.  clips [B, 3, K + horizon, H, W] in
        [-1, 1] as the loader delivers them (horizon defaults to n_frames; longer ones are rolled out like rollout()), labels [B].
        Per clip n_samples futures are drawn, sample s with one z for all its chunks, z from a PRIVATE generator seeded with
        `seed` (neither the default generator nor noise_gen is touched; truncation as in predict()): all n_samples z are drawn
        first, in sample order, and go to the device in one upload before the loop.  Each future goes through
        metrics.frame_metrics(signed=True, quantize=quantize) against the view clips[:, :, K:] -- no denorm pass, no permuted copy
        -- into one device table that is copied to the host once; nothing inside the loop makes the host wait for the device.
        Every future starts from the same generator state: the spectral-norm u / v, which advance with every generator pass even
        in eval mode, are put back after each sample, so sample s is exactly rollout(cond, labels, horizon, z=z_s) and the
        training state (weights, u / v, batch-norm statistics and counters) is bit-equal before and after the call.  -> dict of fp64 numpy arrays:
        psnr, ssim [horizon]: mean over clips and samples; psnr_best, ssim_best [horizon]: mean over clips of the sample with the
        highest horizon-mean of THAT metric (best-of-N, chosen per metric); table: {"mse", "ssim"} [B, n_samples, horizon].
        A frame predicted exactly (mse = 0) has PSNR +inf and makes every mean it enters +inf.
        use_ema / standing_stats as in predict(): the ema_weights() block is entered once around all samples."""
        from . import metrics as M
        K_ = self.n_cond
        horizon = self.n_frames if horizon is None else int(horizon)
        self._rollout_args("evaluate_prediction", clips, horizon, (2, K_ + horizon))
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError(f"n_samples={n_samples}")
        B = clips.shape[0]
        gen = torch.Generator().manual_seed(int(seed))
        clips = to_device_async(clips, self.device).to(torch.float32)
        frames = clips.permute(0, 2, 1, 3, 4)                          # [B, K + horizon, 3, H, W], a view
        cond, target = frames[:, :K_].contiguous(), frames[:, K_:]
        labels_d = to_device_async(self._check_labels(labels), self.device)
        zs = torch.stack([torch.randn(B, self.z_dim, generator=gen) if truncation is None
                          else truncated_z(B, self.z_dim, truncation, generator=gen) for _ in range(n_samples)])
        zs = to_device_async(zs, self.device)                  # [n_samples, B, z_dim]: one upload, before the loop
        mse = torch.empty(n_samples, B, horizon, dtype=torch.float32, device=self.device)
        ssim = torch.empty_like(mse)
        with self._sampling_weights(use_ema, standing_stats, cond, labels):
            frozen = self._g_frozen_tensors()
            saved = [t.clone() for t in frozen]
            self.G.eval()
            try:
                for s in range(n_samples):
                    z = zs[s]
                    raw = self._rollout_raw(cond, labels_d, horizon, lambda: z)
                    M.frame_metrics(raw, target, signed=True, quantize=quantize, out=(mse[s], ssim[s]))
                    for t, old in zip(frozen, saved):
                        t.copy_(old)
            finally:
                self.G.train()
                for t, old in zip(frozen, saved):
                    t.copy_(old)
        table = torch.stack([mse, ssim]).permute(0, 2, 1, 3).cpu().numpy()          # the one copy to the host
        return M.aggregate_prediction(table[0], table[1])

    # ---- distribution distances of generated against real clips (no counterpart in the reference; distmetrics.py)
    def _sample_embedder(self, embed):
        """-> frames [B, T, 3, H, W] (raw [-1, 1], contiguous) -> features [B, d] fp32 on the device."""
        from . import distmetrics as DM
        if callable(embed):
            return lambda frames: embed(frames.permute(0, 2, 1, 3, 4).contiguous())
        if embed == "Dt":
            extract = DM.DiscFeatures(self.D_t)
            return lambda frames: extract(vid_downsample(frames))
        if embed == "Ds":
            extract, T, k = DM.DiscFeatures(self.D_s), self.n_frames, self.k_sample
            ids = (torch.arange(k) * T) // k                          # k evenly spaced frames: no random draw in an evaluation
            return lambda frames: extract(sample_k_frames(frames, T, k, ids))
        raise ValueError(f"embed={embed!r}: \"Dt\", \"Ds\" or a callable clips [B, 3, T, H, W] -> features [B, d]")

    @torch.no_grad()
    def evaluate_samples(self, real, *, n_samples, embed="Dt", batch=None, use_ema=False, standing_stats=None, truncation=None,
                         seed=0, real_stats=None, kid=True, prdc_k=None):
        """Frechet and kernel distance between the features of real clips and of clips generated from noise (n_cond = 0): the
        statistic of FVD / FID / KID (distmetrics.py).  real: a loader or any iterable of (clips [B, 3, T, H, W] in [-1, 1],
        labels [B]); its first n_samples clips are used.  embed: a callable clips [B, 3, T, H, W] -> features [B, d] (fp32, on
        the device; e.g. an I3D network with the published weights gives FVD), or "Dt" / "Ds": the pooled final activation of
        this Trainer's own temporal / spatial discriminator (distmetrics.DiscFeatures; D_t on the downsampled clip, D_s on
        k_sample evenly spaced frames), averaged over the clip.  A DISCRIMINATOR-FEATURE DISTANCE IS COMPARABLE ONLY UNDER ONE
        FIXED DISCRIMINATOR SNAPSHOT: the live D moves with every training step, so compare generator checkpoints, averaged
        against live weights or truncation values with the discriminator of ONE checkpoint loaded, never across training steps.
        As many clips are generated as real ones were read, with the real clips' labels, z from a private generator seeded with
        `seed` (truncation as in sample()), `batch` at a time (default: the first real batch's size), through the generator's
        sampling path: eval mode, use_ema / standing_stats as in sample().  real_stats: FeatureStats of the real set computed
        earlier (FeatureStats.load); the real clips are then embedded only when kid is on.
        -> {"fd", "kid_mean", "kid_std" (None with kid=False), "n_real", "n_fake", "d"}; the KID subsets (100 of 1000 rows,
        clipped to the sample count) are drawn from a private numpy generator seeded with `seed`.
        prdc_k: an int k adds "precision", "recall", "density", "coverage" and "prdc_k" (distmetrics.prdc on the kept features
        of both sets: k = 3 is the precision / recall paper's, k = 5 the density / coverage paper's; the real clips are then
        embedded even when real_stats are given); None (the default) computes, launches and returns exactly what it did without.
        Like rollout() and save_samples() the call leaves no trace: weights, spectral-norm u / v of all three networks, batch-norm
        statistics and every random stream of the training run (torch's default generator included, which a shuffling loader
        draws from when it is iterated) are bit-equal before and after."""
        from . import distmetrics as DM
        if self.n_cond:
            raise RuntimeError("evaluate_samples() measures generation from noise (n_cond = 0); a frame-conditional Trainer has "
                               "evaluate_prediction()")
        n_samples = int(n_samples)
        if n_samples < 2:
            raise ValueError(f"n_samples={n_samples}: a covariance needs at least two clips")
        embedder = self._sample_embedder(embed)
        gen = torch.Generator().manual_seed(int(seed))
        rng_state = torch.get_rng_state()
        if prdc_k is not None and int(prdc_k) < 1:
            raise ValueError(f"prdc_k={prdc_k}")
        keep = kid or prdc_k is not None
        want_real = real_stats is None or keep
        stats_r = stats_f = None
        feats_r, feats_f, labels_all = [], [], []
        n_real = 0
        try:
            for clips, labels in real:
                take = min(clips.shape[0], n_samples - n_real)
                if take <= 0:
                    break
                labels_all.append(self._check_labels(torch.as_tensor(labels)[:take].cpu()))
                if batch is None:
                    batch = clips.shape[0]
                if want_real:
                    frames = to_device_async(clips[:take], self.device).to(torch.float32).permute(0, 2, 1, 3, 4).contiguous()
                    f = embedder(frames)
                    if real_stats is None:
                        if stats_r is None:
                            stats_r = DM.FeatureStats(f.shape[1], self.device)
                        stats_r.update(f)
                    if keep:
                        feats_r.append(f)
                n_real += take
                if n_real >= n_samples:
                    break
        finally:
            torch.set_rng_state(rng_state)
        if n_real < 2:
            raise ValueError(f"`real` delivered {n_real} clips: at least two are needed")
        labels_all = torch.cat(labels_all)
        batch = int(batch)
        if batch < 1:
            raise ValueError(f"batch={batch}")
        with self._sampling_weights(use_ema, standing_stats):
            frozen = self._g_frozen_tensors()
            saved = [t.clone() for t in frozen]
            self.G.eval()
            try:
                for lo in range(0, n_real, batch):
                    y = labels_all[lo:lo + batch]
                    z = (torch.randn(y.shape[0], self.z_dim, generator=gen) if truncation is None
                         else truncated_z(y.shape[0], self.z_dim, truncation, generator=gen))
                    fake = self.G(to_device_async(z, self.device), to_device_async(y, self.device))
                    f = embedder(fake.to(torch.float32).contiguous())
                    if stats_f is None:
                        stats_f = DM.FeatureStats(f.shape[1], self.device)
                    stats_f.update(f)
                    if keep:
                        feats_f.append(f)
            finally:
                self.G.train()
                for t, old in zip(frozen, saved):
                    t.copy_(old)
        ref = real_stats if real_stats is not None else stats_r
        if ref.d != stats_f.d:
            raise ValueError(f"real statistics of width {ref.d} against generated features of width {stats_f.d}")
        out = {"fd": DM.frechet_distance(ref, stats_f), "kid_mean": None, "kid_std": None, "n_real": n_real,
               "n_fake": stats_f.n, "d": stats_f.d}
        if kid:
            res = DM.kid(torch.cat(feats_r), torch.cat(feats_f), seed=int(seed))
            out["kid_mean"], out["kid_std"] = res["mean"], res["std"]
        if prdc_k is not None:
            res = DM.prdc(torch.cat(feats_r), torch.cat(feats_f), k=int(prdc_k))
            out.update({key: res[key] for key in ("precision", "recall", "density", "coverage")}, prdc_k=res["k"])
        return out

    # ---- trainer.py:337-343 / 375-382: reference-compatible checkpoints
    def save_models(self, step):
        """Rank 0 writes (its batch-norm running statistics are the ones saved in "replica" mode); the others wait.
        With a weight average (config.ema_decay > 0) a fourth file `{step}_G_ema.pth` holds G.state_dict() taken inside
        ema_weights(standing_stats=config.ema_standing_stats): the keys of `{step}_G.pth`, loadable into a plain Generator.  A
        frame-conditional Trainer has no context frames at this point: its file carries the averaged weights with the LIVE
        running statistics whatever ema_standing_stats says.  In a data-parallel run every rank enters the block and runs
        the standing-statistics passes (same seed: cross-replica collectives pair up); rank 0 writes."""
        world = D.world_size()
        writer = world == 1 or torch.distributed.get_rank() == 0
        if writer:
            os.makedirs(self.model_save_path, exist_ok=True)
            for net, tag in ((self.G, "G"), (self.D_s, "Ds"), (self.D_t, "Dt")):
                torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()},
                           os.path.join(self.model_save_path, "{}_{}.pth".format(step, tag)))
        if self._ema_on():
            n_pass = 0 if getattr(self, "n_cond", 0) else getattr(self, "ema_standing_stats", 0)
            with self.ema_weights(standing_stats=n_pass):
                if writer:
                    torch.save({k: v.detach().cpu() for k, v in self.G.state_dict().items()},
                               os.path.join(self.model_save_path, "{}_G_ema.pth".format(step)))
        if world > 1:
            torch.distributed.barrier()

    def load_pretrained_model(self):
        for net, tag in ((self.G, "G"), (self.D_s, "Ds"), (self.D_t, "Dt")):
            sd = torch.load(os.path.join(self.model_save_path, "{}_{}.pth".format(self.pretrained_model, tag)),
                            map_location="cpu")
            sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}     # DataParallel prefix
            net.load_state_dict(sd)
        # the average: its own file when there is one, else it starts from the weights just loaded (FlatAdam copies them at
        # the first step)
        path = os.path.join(self.model_save_path, "{}_G_ema.pth".format(self.pretrained_model))
        if self._ema_on() and os.path.exists(path):
            sd = torch.load(path, map_location="cpu")
            sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
            flat = torch.cat([sd[k].reshape(-1).float() for k, p in self.G.named_parameters() if p.requires_grad])
            self.g_optimizer.load_ema(flat.to(self.g_optimizer.flat.device))
