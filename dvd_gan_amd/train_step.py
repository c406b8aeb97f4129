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
Trainer(..., d_cr=lambda_real, d_cr_fake=lambda_fake) adds balanced consistency regularization (Zhao et al. 2020, "Improved
Consistency Regularization for GANs") on those same transforms: in a D iteration every discriminator call takes the transformed
views followed by the clean views of the same clips, and lambda * mean((D(T(x)) - D(x))^2) joins the network's loss (one more
HIP launch per call, functional.CRLoss; the generator step is untouched); `cr_report()` is the one call that reads its statistics.
Trainer(..., z_cr=lambda_dis, z_cr_gen=lambda_gen, z_cr_sigma=sigma) adds the paper's second regularizer, latent consistency
regularization: the generator runs on [z | z + dz], dz ~ N(0, sigma^2), in ONE call on 2B rows; in a D iteration every fake call
takes the views of both halves and z_cr * mean((D(v(G(z))) - D(v(G(z + dz))))^2) joins the network's loss (functional.CRLoss
again); the generator step adds -z_cr_gen * mean((G(z) - G(z + dz))^2) over whole clips (functional.PairDistance: two streaming
HIP launches forward, one backward); `zcr_report()` is the one call that reads its statistics.
`evaluate_samples(real, n_samples=N, embed=...)` measures generation from noise (n_cond = 0): the Frechet and the kernel distance
between features of real and of generated clips (distmetrics.py; the statistic of FVD / FID / KID, on the device).  `embed` is the
caller's feature extractor or "Dt" / "Ds", this Trainer's own discriminator features -- comparable only under ONE fixed
discriminator snapshot.  It leaves no trace in the training state or in any random stream.
Out of scope: tensorboard logging, GIF / MP4 files, dataset loaders.
"""
import os
import time

import torch

from . import functional as Fn
from . import lib as L
from . import dist as D
from . import settings as S
from .augment import ClipAugment, ada_update, draw_params
from .geom_augment import ClipWarp, draw_geom
from .dist import GradExchange
from .disc_nets import SpatialDiscriminator, TemporalDiscriminator
from .gen_net import Generator
from .helpers import draw_frame_ids, sample_k_frames, to_device_async, vid_downsample, vid_downsample_cat
from .optim import FlatAdam
from .trainer_reports import TrainerReports
from .trainer_sampling import TrainerSampling
from .trainer_state import TrainerState


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


class Trainer(TrainerState, TrainerSampling, TrainerReports):
    """The constructor, the step and the training loop; what is written to disk (trainer_state.py), what the generator computes
    outside the step (trainer_sampling.py) and the reports (trainer_reports.py) are plain base classes.  Everything `_train_step`
    calls is defined here or is an instance attribute."""
    # run state, as a Trainer that never ran the constructor finds it (`Trainer.__new__`, a subclass with an `__init__` of its
    # own); the optional config fields get their class-level defaults from settings.SETTINGS below the class
    _adv_ex = False               # a stabiliser or the logit statistics are on: calc_loss takes the AdvLossEx launch
    _adv_stats = None             # fp32 [6][lib.ADV_NSTAT]: D_s real / fake, D_t real / fake, G step D_s / D_t
    _anchors = None               # fp32 [2 slots][D_s, D_t][real, fake] on the device, when lecam > 0
    d_cr = 0.0                    # weights of the consistency penalty on real / on generated clips (constructor keywords)
    d_cr_fake = 0.0
    _cr_stats = None              # fp32 [4][lib.CR_NSTAT]: D_s real / fake, D_t real / fake, when either weight is > 0
    z_cr = 0.0                    # weights of latent consistency regularization on D_s / D_t and on G, scale of the perturbation
    z_cr_gen = 0.0
    z_cr_sigma = 0.03
    _zcr_stats = None             # fp32 [2][lib.CR_NSTAT]: D_s, D_t fake calls, when z_cr or z_cr_gen is > 0 ...
    _zcr_stats_g = None           # ... and fp32 [lib.ZCR_NSTAT] of the generator step
    _ema_block = False            # inside ema_weights()
    _epoch = 0                    # epochs train() has started
    _labels_registered = None     # register_label_buffer()'s tensor
    _sheets = None                # the sheets.SheetWriter, made at first use
    _state_writer = None          # the checkpoint.StateWriter, made at the first save_state()
    g_optimizer = None

    def __init__(self, data_loader, config, device=None, compute_dtype=torch.bfloat16, latent_dim=4, dp_mode="replica", rnn="gru",
                 tsru_flow=2.0, d_cr=0.0, d_cr_fake=None, z_cr=0.0, z_cr_gen=0.0, z_cr_sigma=0.03):
        """dp_mode (data-parallel runs only): "replica" = per-replica batch-norm statistics and condition rows, the
        semantics of the reference's nn.DataParallel (trainer.py:353-359); "global" = cross-replica conditional batch
        norm + gathered conditions: N ranks reproduce one process on the global batch.
        rnn, tsru_flow: the generator's recurrent unit and its flow range (gen_net.Generator); an architecture choice like
        latent_dim, so a keyword here and no config field.
        d_cr, d_cr_fake: the weights lambda_real and lambda_fake of balanced consistency regularization (Zhao et al. 2020; the
        paper uses 10 for both): in a D iteration each discriminator is asked to give a clip and its d_aug / d_aug_geom view the
        same logit, L_D += d_cr * mean((D(T(x)) - D(x))^2) + d_cr_fake * mean((D(T(G(z))) - D(G(z)))^2).  0 = off; d_cr_fake =
        None takes d_cr.  They steer future steps only: neither the fingerprint nor the state file knows them.  In a data-parallel
        run the penalty is a mean over the rank's shard, which the gradient exchange turns into the mean over the global batch
        when the shards are equal (unverified, like every other stabiliser there).
        z_cr, z_cr_gen, z_cr_sigma: latent consistency regularization of the same paper (its ICR = bCR + zCR).  With z' = z + dz,
        dz ~ N(0, z_cr_sigma^2): in a D iteration L_D += z_cr * mean((D(v(G(z))) - D(v(G(z'))))^2) for each discriminator, v being
        whatever the step applies to generated clips (frame sampling / downsampling, d_aug / d_aug_geom with the same frame ids
        and table rows for both members of a pair); in the generator step L_G += -z_cr_gen * mean((G(z) - G(z'))^2) over all
        elements of the B clips, before any view.  As reported for the paper's BigGAN runs: lambda_dis = 5, lambda_gen = 0.5,
        sigma = 0.03.  0 / 0 = off (the default): nothing is allocated, drawn or launched.  With either weight > 0 the generator
        runs on 2B rows [z | z'] in one call, dz is drawn from the noise generator right after z_class (draws["z_delta"] in a test),
        and zcr_report() reads the statistics; sigma = 0 gives identical pairs.  The six returned losses do not change: the
        generator's term is reported like ortho_penalty.  They steer future steps only (no fingerprint, no state: the noise
        generator is saved already).  Data parallel as for d_cr: shard means averaged by the gradient exchange, unverified."""
        if dp_mode not in ("replica", "global"):
            raise ValueError("dp_mode must be 'replica' or 'global'")
        if rnn not in ("gru", "tsru"):
            raise ValueError(f"rnn={rnn!r}: the recurrent unit is 'gru' or 'tsru'")
        from .gen_net import check_tsru_flow
        check_tsru_flow(tsru_flow)
        d_cr = float(d_cr)
        d_cr_fake = d_cr if d_cr_fake is None else float(d_cr_fake)
        if not (0.0 <= d_cr < float("inf") and 0.0 <= d_cr_fake < float("inf")):
            raise ValueError(f"d_cr={d_cr}, d_cr_fake={d_cr_fake}: the consistency weights are finite and >= 0")
        self.d_cr, self.d_cr_fake = d_cr, d_cr_fake
        z_cr, z_cr_gen, z_cr_sigma = float(z_cr), float(z_cr_gen), float(z_cr_sigma)
        if not (0.0 <= z_cr < float("inf") and 0.0 <= z_cr_gen < float("inf") and 0.0 <= z_cr_sigma < float("inf")):
            raise ValueError(f"z_cr={z_cr}, z_cr_gen={z_cr_gen}, z_cr_sigma={z_cr_sigma}: the latent consistency weights and the "
                             "scale of the perturbation are finite and >= 0")
        self.z_cr, self.z_cr_gen, self.z_cr_sigma = z_cr, z_cr_gen, z_cr_sigma
        self.rnn, self.tsru_flow = rnn, float(tsru_flow)
        self.dp_mode = dp_mode
        self.data_loader = data_loader
        c = self.config = config
        self.adv_loss, self.z_dim = c.adv_loss, c.z_dim
        self.g_chn, self.ds_chn, self.dt_chn = c.g_chn, c.ds_chn, c.dt_chn
        self.n_frames, self.lr_schr = c.n_frames, c.lr_schr
        self.total_epoch, self.d_iters, self.batch_size = c.total_epoch, c.d_iters, c.batch_size
        self.g_lr, self.d_lr, self.beta1, self.beta2 = c.g_lr, c.d_lr, c.beta1, c.beta2
        self.n_class, self.k_sample = c.n_class, c.k_sample
        # every optional field (settings.SETTINGS: attribute, field, cast, default); the groups are explained at their checks below
        for attr, field, cast, default in S.SETTINGS:
            setattr(self, attr, cast(getattr(c, field, default)))
        self.model_save_path = os.path.join(getattr(c, "model_save_path", "./models"), getattr(c, "version", ""))
        self.sample_path = os.path.join(getattr(c, "sample_path", "./samples"), getattr(c, "version", ""))
        if self.n_cond < 0:
            raise ValueError(f"n_cond={self.n_cond}")
        if self.n_cond and (self.n_cond + self.n_frames) % 4:
            # D_t sees context + generated frames and pools time twice (TemporalDiscriminator._forward)
            raise ValueError(f"n_cond + n_frames = {self.n_cond + self.n_frames} must be a multiple of 4: D_t judges the context "
                             "and the generated frames together and pools time twice")
        # generator weight average (0 = off): decay, steps it merely follows the weights, standing-statistics passes at
        # sampling / saving time and the seed of their private noise generator
        if not 0.0 <= self.ema_decay < 1.0 or self.ema_start < 0 or self.ema_standing_stats < 0:
            raise ValueError(f"ema_decay={self.ema_decay} (in [0, 1)), ema_start={self.ema_start}, "
                             f"ema_standing_stats={self.ema_standing_stats} (both >= 0)")
        # orthogonal regularization of the generator's matrices (0 = off): strength beta of g += beta * 2 M W
        if not 0.0 <= self.g_ortho < float("inf"):
            raise ValueError(f"g_ortho={self.g_ortho} must be a finite strength >= 0")
        # gradient guard (all 0 / False = off): clipping norms of G and of the two discriminators, skipping of non-finite steps,
        # rows of the per-network norm log
        if not (0.0 <= self.g_clip_norm < float("inf") and 0.0 <= self.d_clip_norm < float("inf")) or self.grad_log < 0:
            raise ValueError(f"g_clip_norm={self.g_clip_norm}, d_clip_norm={self.d_clip_norm} (finite norms >= 0), "
                             f"grad_log={self.grad_log} (rows >= 0)")
        # stabilisers and diagnostics on the discriminators' logits (all 0 / False = off: calc_loss is then the plain launch).
        # LeCam regularization: strength, decay of the logit anchors, first D iteration the gradient applies in (the anchors
        # accumulate from the first one); top-k generator updates: floor nu of the kept fraction, its decay per epoch; the
        # logit statistics behind d_stats()
        if (not 0.0 <= self.lecam < float("inf") or not 0.0 <= self.lecam_decay < 1.0 or self.lecam_start < 0
                or not 0.0 <= self.g_topk <= 1.0 or not 0.0 < self.g_topk_decay <= 1.0):
            raise ValueError(f"lecam={self.lecam} (finite, >= 0), lecam_decay={self.lecam_decay} (in [0, 1)), "
                             f"lecam_start={self.lecam_start} (>= 0), g_topk={self.g_topk} (in [0, 1]), "
                             f"g_topk_decay={self.g_topk_decay} (in (0, 1])")
        # augmentation of what the discriminators see (d_aug = "" = off: no table, no generator, no launch): the groups of
        # augment.POLICIES, the probability a group applies to a clip with, the r_t it is steered towards (0 = fixed p), steps
        # between two adjustments, thousands of real clips in which p crosses [0, 1], seed of the tables' private generator
        # ... and d_aug_geom the geometric groups of geom_augment.GEOM_POLICIES, applied before them; every other setting is shared.
        # d_aug_p is the current p: adaptive runs move it (d_aug_target > 0)
        if (not 0.0 <= self.d_aug_p <= 1.0 or not 0.0 <= self.d_aug_target < 1.0 or self.d_aug_interval < 1
                or not 0.0 < self.d_aug_kimg < float("inf")):
            raise ValueError(f"d_aug_p={self.d_aug_p} (in [0, 1]), d_aug_target={self.d_aug_target} (in [0, 1), 0 = fixed p), "
                             f"d_aug_interval={self.d_aug_interval} (>= 1), d_aug_kimg={self.d_aug_kimg} (finite, > 0)")
        if (self.d_cr > 0.0 or self.d_cr_fake > 0.0) and not (self.d_aug or self.d_aug_geom):
            raise ValueError(f"d_cr={self.d_cr}, d_cr_fake={self.d_cr_fake} with d_aug and d_aug_geom both empty: there is no "
                             "transform for the discriminators to be consistent under")
        self._aug_adaptive = bool(self.d_aug or self.d_aug_geom) and self.d_aug_target > 0.0
        self._aug_gen = None          # the tables' generator, made below once the rank is known
        self._aug_steps = 0           # steps taken with d_aug or d_aug_geom on
        self._aug_adjustments = 0     # adjustments of p made
        self._adv_ex = self.lecam > 0.0 or self.g_topk > 0.0 or self._d_stats_on or self._aug_adaptive
        self._lecam_it = 0            # D iterations done
        # singular-value monitoring of the weights (sv_log = 0 = off: no table, no workspace, no launch): every sv_log-th step
        # sv_iters more block power iterations on each network's monitor and one row of its device ring of sv_log_rows rows; top
        # sv_k values from blocks of sv_block columns, start blocks from a private generator seeded with sv_seed (spectral.py)
        if (self.sv_log < 0 or not 1 <= self.sv_iters <= L.SV_MAX_ITERS or self.sv_log_rows < 1
                or not 1 <= self.sv_k <= self.sv_block <= L.SV_MAX_BLOCK):
            raise ValueError(f"sv_log={self.sv_log} (>= 0), sv_iters={self.sv_iters} (in [1, {L.SV_MAX_ITERS}]), "
                             f"sv_log_rows={self.sv_log_rows} (>= 1), sv_k={self.sv_k}, sv_block={self.sv_block} "
                             f"(1 <= sv_k <= sv_block <= {L.SV_MAX_BLOCK})")
        self._sv = None               # {"G", "Ds", "Dt"} -> spectral.SpectrumMonitor, made at first use
        self._sv_steps = 0            # steps this Trainer has taken
        self._sv_logged = []          # step numbers of the rows logged so far
        # exact resume (all unset = off: no thread, no allocation, no file): a full training state every state_save_step steps
        # as `{step}_state.pt`, the newest state_keep of them kept (0 = all); resume = a state file or "latest"
        if self.state_save_step < 0 or self.state_keep < 0:
            raise ValueError(f"state_save_step={self.state_save_step}, state_keep={self.state_keep} (both >= 0)")
        if self.resume and self.pretrained_model:
            raise ValueError(f"resume={self.resume!r} and pretrained_model={self.pretrained_model!r}: a run continues either from a "
                             "full training state or from reference-format weights, not from both")
        self._resumed_step = None    # the step of the state load_state() read
        # sample sheets (sample_step = sample_epoch = 0: off): period in steps, or in epochs like the reference (trainer.py:186);
        # directory (trainer.py:69); clips per class; "frames" = a PNG per clip, "clips" = one animation of all clips, "both"
        if (self.sample_step < 0 or self.sample_epoch < 0 or self.test_batch_size < 1 or not self.sample_fps > 0
                or self.sample_layout not in ("frames", "clips", "both")):
            raise ValueError(f"sample_step={self.sample_step}, sample_epoch={self.sample_epoch} (>= 0), "
                             f"test_batch_size={self.test_batch_size} (>= 1), sample_fps={self.sample_fps} (> 0), "
                             f"sample_layout={self.sample_layout!r} ('frames' | 'clips' | 'both')")
        self._fixed = None            # fixed_inputs(), drawn at first use
        self.device = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.compute_dtype, self.latent_dim = compute_dtype, latent_dim
        if self._adv_ex:
            self._adv_stats = torch.zeros(6, L.ADV_NSTAT, dtype=torch.float32, device=self.device)
            if self.lecam > 0.0:
                self._anchors = torch.zeros(2, 2, 2, dtype=torch.float32, device=self.device)
        if self.d_cr > 0.0 or self.d_cr_fake > 0.0:
            self._cr_stats = torch.zeros(4, L.CR_NSTAT, dtype=torch.float32, device=self.device)
        if self.z_cr > 0.0 or self.z_cr_gen > 0.0:
            self._zcr_stats = torch.zeros(2, L.CR_NSTAT, dtype=torch.float32, device=self.device)
            self._zcr_stats_g = torch.zeros(L.ZCR_NSTAT, dtype=torch.float32, device=self.device)
        Fn.direct_weight_grads(True)         # weight gradients accumulate into FlatAdam's buffers on a side stream
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

    def _d_tables(self, draws, B_real, H, W):
        """The four tables of one D iteration on the device, in the order they are drawn: the parameter tables [B, lib.AUG_COLS]
        "aug_real" and "aug_fake", then the tables of warps [B, lib.GEOM_COLS] "geom_real" and "geom_fake"; None for a stage that
        is off.  One table for the real clips and an independent one for the fake clips; both discriminators see the same
        transform of a clip (the frame gather and the 2 x 2 average work on the augmented clip).  Each is draws[key] (test aid)
        or a draw from the private generator; the warps' tables come after the others: a run without d_aug_geom draws what it
        drew before."""
        B_fake = self.batch_size if draws is None else len(draws["z"])
        out = []
        for name, policy, cols, draw in (("aug", self.d_aug, L.AUG_COLS, draw_params),
                                         ("geom", self.d_aug_geom, L.GEOM_COLS, draw_geom)):
            for key, B in ((name + "_real", B_real), (name + "_fake", B_fake)):
                if not policy:
                    out.append(None)
                    continue
                if draws is not None and key in draws:
                    tab = torch.as_tensor(draws[key], dtype=torch.float32).reshape(B, cols).contiguous()
                else:
                    tab = draw(B, H, W, policy, self.d_aug_p, self._aug_gen)
                out.append(to_device_async(tab, self.device))
        return out

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

    def _sv_log_row(self):
        row = len(self._sv_logged) % self.sv_log_rows
        for mon in self._sv_monitors().values():
            mon.update(self.sv_iters).snapshot(row)
        self._sv_logged.append(self._sv_steps)

    # ---- trainer.py:345-366
    def build_model(self):
        dt = self.compute_dtype
        self.G = Generator(self.z_dim, self.latent_dim, self.n_class, self.g_chn, self.n_frames, compute_dtype=dt,
                           self_attn=self.g_self_attn, sep_attn=self.g_sep_attn, n_cond=self.n_cond, rnn=self.rnn,
                           tsru_flow=self.tsru_flow).to(self.device)
        self.D_s = SpatialDiscriminator(self.ds_chn, self.n_class, compute_dtype=dt).to(self.device)
        self.D_t = TemporalDiscriminator(self.dt_chn, self.n_class, compute_dtype=dt).to(self.device)
        if self.exchange.active and self.dp_mode == "global":
            from .sn_layers import ConditionalNorm
            self.G.dp_global = True
            for m in self.G.modules():
                if isinstance(m, ConditionalNorm):
                    m.replicas = (self.exchange.world, D.all_reduce_sum_)
        self.select_opt_schr()

    def _nets(self):
        return (("G", self.G), ("Ds", self.D_s), ("Dt", self.D_t))

    def _optimizers(self):
        return (("G", self.g_optimizer), ("Ds", self.ds_optimizer), ("Dt", self.dt_optimizer))

    def _schedulers(self):
        return (("G", self.g_lr_scher), ("Ds", self.ds_lr_scher), ("Dt", self.dt_lr_scher))

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
        if _site is None or not self._adv_ex:
            return Fn.AdvLoss.apply(x, bool(real_flag), self.adv_loss == "hinge")
        group = x.numel() // self._cur_B               # k_sample for D_s, frames / 4 for D_t: the logits are sample-major
        keep, lecam, anchors = 0, 0.0, None
        if _site >= 4:
            if self.g_topk > 0.0:                      # (train() counts the epochs it has started: the running one is _epoch - 1)
                keep = topk_keep(self._cur_B, self.g_topk, self.g_topk_decay, max(0, self._epoch - 1))
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
        return self.calc_loss(x, real_flag, _site=site) if self._adv_ex else self.calc_loss(x, real_flag)

    def _d_pair(self, net, view, partners, labels, real_flag, site):
        """One discriminator call of a D iteration with a consistency penalty on -> (adversarial term, sum of the penalties).
        partners: a list of (clips, weight, statistics row), each a group the size of `view` that the network is asked to score
        like `view` -- the clean views of the same clips (balanced consistency regularization: d_cr / d_cr_fake, a row of
        _cr_stats), the views of the clips of the perturbed latents (latent consistency regularization: z_cr, a row of
        _zcr_stats).  All groups go through ONE call on a batch 1 + len(partners) times as long (both networks are per-sample, no
        batch norm), so the spectral-norm vectors advance once per call as without a penalty.  The first group's logits are what
        the call returns today and go through _site_loss unchanged; each penalty is weight * mean((first - group)^2)
        (functional.CRLoss)."""
        out = net(torch.cat([view] + [p[0] for p in partners]), torch.cat([labels] * (1 + len(partners))))
        n = out.numel() // (1 + len(partners))
        penalty = None
        for i, (_, weight, stats) in enumerate(partners):
            term = Fn.CRLoss.apply(out[:n], out[(i + 1) * n:(i + 2) * n], weight, stats)
            penalty = term if penalty is None else penalty + term
        return self._site_loss(out[:n], real_flag, site), penalty

    def _end_d_iteration(self):
        """The anchors of the slot this D iteration wrote become those of the global batch (the update is linear in the batch
        mean and the shards are equal): one all-reduce of 4 floats, only in a data-parallel run."""
        if self._anchors is None:
            return
        if self.exchange.active:
            cur = self._anchors[self._lecam_it & 1]
            buf = cur.to(D.collective_device())
            torch.distributed.all_reduce(buf, op=torch.distributed.ReduceOp.SUM)
            cur.copy_(buf / D.world_size())
        self._lecam_it += 1

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
        if labels.is_cuda and self._labels_registered is labels and self._labels_version == labels._version:
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
        all K+T frames.  With z_cr or z_cr_gen on, `draws` also holds "z_delta" [B, z_dim], the perturbation of z itself.
        Returns the six loss terms as device scalars:
        ds_real, ds_fake, dt_real, dt_fake, g_s, g_t.
        The step's dependent chain runs on a HIGH-priority stream so its (often small) launches are dispatched ahead of
        the bulk weight-gradient work queued on the normal-priority side stream; the caller's stream is ordered before
        and after the step, so nothing changes for it."""
        if self._zcr_stats is not None and draws is not None:
            for d in draws if isinstance(draws, (list, tuple)) else (draws,):
                d["z_delta"]                                      # pinned draws pin the perturbation too: KeyError before any launch
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
        aug, geo = bool(self.d_aug), bool(self.d_aug_geom)
        cr = self._cr_stats is not None
        zcr = self._zcr_stats is not None
        tab_real = tab_fake = mat_real = mat_fake = None
        for _ in range(self.d_iters):
            if isinstance(draws_all, (list, tuple)):              # test aid: one dict of draws per discriminator iteration
                draws = draws_all[_]
            ids_real = draw_frame_ids(T, k, fg) if draws is None else torch.as_tensor(draws["perm_real"])[:k].sort()[0]
            # (with the consistency penalty on, the real passes stay on the chain: the opt-in side-stream path is not taken)
            early = self._aux is not None and not cr
            real_in = real_videos
            if aug or geo:
                tab_real, tab_fake, mat_real, mat_fake = self._d_tables(draws, real_videos.shape[0], *real_videos.shape[-2:])
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
            if zcr:
                # latent consistency regularization: ONE generator call on [z | z + dz] (labels, context and states repeated), so
                # the spectral-norm vectors and the batch-norm counters advance once; rows [:B] are the base clips (everything the
                # step did with the generator's output, it does with them), rows [B:] their partners
                z_delta = to_device_async(self.z_cr_sigma * torch.randn(self.batch_size, self.z_dim, generator=self.noise_gen)
                                          if draws is None else torch.as_tensor(draws["z_delta"]), self.device)
                B = z.shape[0]
                twice = (lambda t: None if t is None else torch.cat([t, t]))
                fake_both = self.G(torch.cat([z, z + z_delta]), twice(z_class),
                                   None if hidden is None else [h if h is None else [twice(s) for s in h] for h in hidden],
                                   cond=twice(cond))
                fake_videos, fake_part = fake_both[:B], fake_both[B:].detach()
            else:
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
            if zcr:
                # the partners' views: the same table rows, the same frame ids (and below the same context views)
                part_in = self._d_view(fake_part, mat_fake, tab_fake) if aug or geo else fake_part
            # ---------------- D_s
            if early:
                cur.wait_stream(self._aux)
                for t_ in (ds_loss_real, dt_loss_real, real_d):
                    t_.record_stream(cur)
            elif cr:
                # balanced consistency regularization: every discriminator call of the D iteration takes [transformed | clean]
                # views of the same clips (the same frame ids), and the penalties join the network's loss before its one backward
                ds_loss_real, ds_cr_real = self._d_pair(
                    self.D_s, real_s, [(sample_k_frames(real_videos, T + Kc, k, ids_real + Kc if Kc else ids_real), self.d_cr,
                                        self._cr_stats[0])], real_labels, True, 0)
            else:
                ds_loss_real = self._site_loss(self.D_s(real_s, real_labels), True, 0)
            if cr or zcr:
                # the fake call's groups: [T(base) | clean base (d_cr_fake) | T(partners) (z_cr)]
                partners = []
                if cr:
                    fake_clean = fake_videos.detach()
                    partners.append((sample_k_frames(fake_clean, T, k, ids_fake), self.d_cr_fake, self._cr_stats[1]))
                if zcr:
                    partners.append((sample_k_frames(part_in, T, k, ids_fake), self.z_cr, self._zcr_stats[0]))
                ds_loss_fake, ds_cr_fake = self._d_pair(self.D_s, fake_s.detach(), partners, z_class, False, 1)
            else:
                ds_loss_fake = self._site_loss(self.D_s(fake_s.detach(), z_class), False, 1)
            self.reset_grad()
            ds_loss = ds_loss_real + ds_loss_fake
            if cr:
                ds_loss = ds_loss + ds_cr_real
            if cr or zcr:
                ds_loss = ds_loss + ds_cr_fake
            ds_loss.backward()
            Fn.join_side()
            ex.start("Ds", self.ds_optimizer.grad)
            # ---------------- D_t (its forward/backward overlaps the D_s gradient exchange)
            fake_d = vid_downsample(fake_in) if cond is None else vid_downsample_cat(cond_in, fake_in)
            if cr:
                dt_loss_real, dt_cr_real = self._d_pair(self.D_t, vid_downsample(real_in),
                                                        [(vid_downsample(real_videos), self.d_cr, self._cr_stats[2])], real_labels, True, 2)
            elif not early:
                real_d = vid_downsample(real_in)
                dt_loss_real = self._site_loss(self.D_t(real_d, real_labels), True, 2)
            if cr or zcr:
                partners = []
                if cr:
                    # the clean view of the fake call is [raw context | generated]
                    partners.append((vid_downsample(fake_clean) if cond is None else vid_downsample_cat(cond, fake_clean),
                                     self.d_cr_fake, self._cr_stats[3]))
                if zcr:
                    partners.append((vid_downsample(part_in) if cond is None else vid_downsample_cat(cond_in, part_in),
                                     self.z_cr, self._zcr_stats[1]))
                dt_loss_fake, dt_cr_fake = self._d_pair(self.D_t, fake_d.detach(), partners, z_class, False, 3)
            else:
                dt_loss_fake = self._site_loss(self.D_t(fake_d.detach(), z_class), False, 3)
            ex.finish("Ds")
            self.ds_optimizer.step()
            self.ds_lr_scher.step((ds_loss_real + ds_loss_fake) if self._plateau else None)
            self.dt_optimizer.zero_grad()
            dt_loss = dt_loss_real + dt_loss_fake
            if cr:
                dt_loss = dt_loss + dt_cr_real
            if cr or zcr:
                dt_loss = dt_loss + dt_cr_fake
            dt_loss.backward()
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
        if zcr and self.z_cr_gen > 0.0:
            # the generator is asked not to map z and z + dz to the same clip: the one term that reads both halves of its output
            (g_s_loss + g_t_loss + Fn.PairDistance.apply(fake_both, self.z_cr_gen, self._zcr_stats_g)).backward()
        else:
            if zcr:                                           # z_cr_gen = 0: the distances are still reported
                with torch.no_grad():
                    Fn.PairDistance.apply(fake_both.detach(), 0.0, self._zcr_stats_g)
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
        if self.sv_log:
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
        state_save_step = self.state_save_step
        self.D_s.train(); self.D_t.train(); self.G.train()
        t0 = time.time()
        # sample sheets: every sample_step steps, or every sample_epoch epochs (trainer.py:186); 0 = never, nothing is set up
        sample_step = self.sample_step or int(self.sample_epoch * steps_per_epoch)
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
                    rep = self.d_stats()
                    for tag in ("Ds", "Dt") if rep else ():
                        line += ", %s r_t: %.3f lecam: %.3e/%.3e" % (tag, rep[tag]["r_t"], rep[tag]["lecam_real"],
                                                                     rep[tag]["lecam_fake"])
                    if self.d_aug or self.d_aug_geom:
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


# the class-level default of every optional config field, one per row of the settings table
for _attr, _value in S.DEFAULTS.items():
    setattr(Trainer, _attr, _value)
