"""What a Trainer computes with its generator outside the training step: samples, predictions, rollouts, their evaluation and the
sample sheets (trainer.py:195-197, 323-334, 389-391; sheets.py, metrics.py, distmetrics.py), with the live or the averaged
weights.  A plain base class of train_step.Trainer.  `_g_eval()` is the ONE statement of what "a generator pass that leaves no
trace" restores; `ema_weights()` keeps a restore of its own (it also puts back momenta and the mode it found)."""
import contextlib
import os

import torch

from . import dist as D
from . import kern as K
from .helpers import denorm, sample_k_frames, to_device_async, truncated_z, vid_downsample


class TrainerSampling(object):
    # ---- the averaged generator weights
    def _ema_on(self):
        return bool(self.g_optimizer is not None and self.g_optimizer.ema_decay)

    def _g_frozen_tensors(self):
        """Every tensor of G that Adam does not own: spectral-norm u / v, batch-norm running statistics and counters."""
        return [p.data for p in self.G.parameters() if not p.requires_grad] + list(self.G.buffers())

    @contextlib.contextmanager
    def _g_eval(self, restore=True):
        """Inside the block G is in eval mode; on exit, with or without an exception, it is back in train mode.  restore=True:
        every tensor of `_g_frozen_tensors()` is cloned on entry and copied back on exit, and the block yields `put_back()`, which
        copies them back in between (after a pass, so that the next one starts from the same state): the generator passes
        inside leave no trace.  restore=False (sample(), predict()): nothing is cloned, `put_back()` does nothing and the
        spectral-norm u / v keep what the passes made of them (quirk 2).  Enter it INSIDE `_sampling_weights(...)`: after the
        weight exchange and the standing-statistics passes."""
        frozen = self._g_frozen_tensors() if restore else ()
        saved = [t.clone() for t in frozen]

        def put_back():
            for t, old in zip(frozen, saved):
                t.copy_(old)

        self.G.eval()
        try:
            yield put_back
        finally:
            self.G.train()
            put_back()

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
        if self._ema_block:
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

    def _draw_z(self, batch, truncation, generator=None):
        """z [batch, z_dim] on the host, truncated to [-truncation, truncation] when that is given; generator=None draws from
        noise_gen (a single process: the default generator)."""
        generator = self.noise_gen if generator is None else generator
        if truncation is None:
            return torch.randn(batch, self.z_dim, generator=generator)
        return truncated_z(batch, self.z_dim, truncation, generator=generator)

    # ---- trainer.py:323-334: the sampling path (eval-mode G on fixed z / labels, BN running statistics); the image files are
    # save_samples() below (tensorboard stays out)
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
        with self._sampling_weights(use_ema, standing_stats), self._g_eval(restore=False):
            fake = self.G(fixed_z.to(self.device), fixed_label.to(self.device))
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
        with self._sampling_weights(use_ema, standing_stats, cond, labels), self._g_eval(restore=False):
            fake = self.G(z.to(self.device), self._check_labels(labels).to(self.device), cond=cond.to(self.device, torch.float32))
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
        with self._sampling_weights(use_ema, standing_stats, cond, labels), self._g_eval():
            raw = self._rollout_raw(cond.to(self.device, torch.float32),
                                    to_device_async(self._check_labels(labels), self.device), int(horizon), draw)
        return denorm(raw)

    def _prediction_inputs(self, what, clips, labels, horizon, n_samples, seed, truncation=None):
        """What evaluate_prediction() and save_predictions() start from: the checked (horizon, n_samples), the clips as the view
        frames [B, K + horizon, 3, H, W] on the device in fp32, the contiguous context frames cond, the labels on the device and
        zs [n_samples, B, z_dim]: all z drawn first, in sample order, from a private generator seeded with `seed`, one upload."""
        K_ = self.n_cond
        horizon = self.n_frames if horizon is None else int(horizon)
        self._rollout_args(what, clips, horizon, (2, K_ + horizon))
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError(f"n_samples={n_samples}")
        B = clips.shape[0]
        gen = torch.Generator().manual_seed(int(seed))
        clips = to_device_async(clips, self.device).to(torch.float32)
        frames = clips.permute(0, 2, 1, 3, 4)                          # [B, K + horizon, 3, H, W], a view
        cond = frames[:, :K_].contiguous()
        labels_d = to_device_async(self._check_labels(labels), self.device)
        zs = to_device_async(torch.stack([self._draw_z(B, truncation, gen) for _ in range(n_samples)]), self.device)
        return horizon, n_samples, frames, cond, labels_d, zs

    def _futures(self, cond, labels_d, horizon, zs, put_back):
        """(s, raw future s [B, horizon, 3, H, W]) for every z of zs, each from the same generator state: the caller consumes
        the clip, then u / v are put back before the next pass."""
        for s in range(zs.shape[0]):
            z = zs[s]
            yield s, self._rollout_raw(cond, labels_d, horizon, lambda: z)
            put_back()

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
        horizon, n_samples, frames, cond, labels_d, zs = self._prediction_inputs("evaluate_prediction", clips, labels, horizon,
                                                                                  n_samples, seed, truncation)
        target = frames[:, self.n_cond:]
        mse = torch.empty(n_samples, frames.shape[0], horizon, dtype=torch.float32, device=self.device)
        ssim = torch.empty_like(mse)
        with self._sampling_weights(use_ema, standing_stats, cond, labels), self._g_eval() as put_back:
            for s, raw in self._futures(cond, labels_d, horizon, zs, put_back):
                M.frame_metrics(raw, target, signed=True, quantize=quantize, out=(mse[s], ssim[s]))
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
        with self._sampling_weights(use_ema, standing_stats), self._g_eval():
            for lo in range(0, n_real, batch):
                y = labels_all[lo:lo + batch]
                z = self._draw_z(y.shape[0], truncation, gen)
                fake = self.G(to_device_async(z, self.device), to_device_async(y, self.device))
                f = embedder(fake.to(torch.float32).contiguous())
                if stats_f is None:
                    stats_f = DM.FeatureStats(f.shape[1], self.device)
                stats_f.update(f)
                if keep:
                    feats_f.append(f)
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

    # ---- the Inception Score and class fidelity of generated clips under the caller's classifier (no counterpart in the reference;
    # classmetrics.py)
    @torch.no_grad()
    def evaluate_classes(self, classifier, *, n_samples, labels=None, real=None, batch=None, splits=10, fidelity=True,
                         confusion=False, use_ema=False, standing_stats=None, truncation=None, seed=0):
        """Inception Score and class fidelity of n_samples clips generated from noise (n_cond = 0) under `classifier`: any callable
        clips [B, 3, T, H, W] in [-1, 1] -> logits [B, C] (fp32, bf16 or fp16) on the device; a C3D network fine-tuned on UCF-101
        gives the Inception Score video GANs publish.  The clips are conditioned on the first of: `labels` [n_samples]; the labels
        of the first n_samples clips of `real` (a loader or any iterable of (clips [B, 3, T, H, W] in [-1, 1], labels [B]), which
        must deliver that many); arange(n_samples) % n_class, balanced and drawn from nothing.  z comes from a private generator
        seeded with `seed` (truncation as in sample()), `batch` clips at a time (default: batch_size), through the generator's
        sampling path: eval mode, use_ema / standing_stats as in sample().  No logits are kept: every batch goes straight into a
        classmetrics.LogitStats of `splits` splits.
        fidelity=True compares the argmax with the conditioning labels (top1, top5, mean_log_lik; confusion=True: the matrix and
        per_class_top1 too) and needs the classifier's classes to BE the generator's: a label >= C is a ValueError before anything
        is generated.  C is learned from the first real batch when `real` is given, else from one call of the classifier on a single
        all-zero clip.  fidelity=False serves a classifier over another label set (the Inception Score alone).
        With `real` the same classifier scores the real clips against their own labels and their metrics come back as real_<key>:
        the ceiling of every number here, which papers quote beside the generated one.
        -> the dict of LogitStats.result() (is_mean, is_std, is_all, h_marginal, h_conditional, n, n_bad, n_bad_label, confusion,
        with fidelity top1, top5, mean_log_lik, per_class_top1), the real_<key> entries and "n_classes".
        Like evaluate_samples() the call leaves no trace: weights, spectral-norm u / v of all three networks, batch-norm statistics
        and every random stream of the training run (noise_gen and torch's default generator included) are bit-equal before and
        after."""
        from . import classmetrics as CM
        if self.n_cond:
            raise RuntimeError("evaluate_classes() measures generation from noise (n_cond = 0); a frame-conditional Trainer has "
                               "evaluate_prediction()")
        n_samples = int(n_samples)
        if n_samples < 1:
            raise ValueError(f"n_samples={n_samples}")
        splits = int(splits)
        if not 1 <= splits <= n_samples:
            raise ValueError(f"splits={splits}: 1 to n_samples={n_samples}")
        batch = int(self.batch_size if batch is None else batch)
        if batch < 1:
            raise ValueError(f"batch={batch}")
        if confusion and not fidelity:
            raise ValueError("confusion=True compares with the conditioning labels: it needs fidelity=True")
        if labels is not None:
            labels = self._check_labels(torch.as_tensor(labels).cpu().to(torch.long))
            if labels.dim() != 1 or labels.shape[0] != n_samples:
                raise ValueError(f"labels {tuple(labels.shape)} must hold n_samples={n_samples} class ids")
        gen = torch.Generator().manual_seed(int(seed))

        def score(stats, clips, y):
            logits = classifier(clips)
            if stats is None:
                stats = CM.LogitStats(logits.shape[1], n_samples, splits=splits, confusion=confusion, device=self.device)
            return stats.update(logits, y if fidelity else None)

        out, n_classes = {}, None
        if real is not None:
            stats_r, real_labels, n_real = None, [], 0
            rng_state = torch.get_rng_state()                  # a shuffling loader draws from the default generator
            try:
                for clips, y in real:
                    take = min(clips.shape[0], n_samples - n_real)
                    if take <= 0:
                        break
                    y = torch.as_tensor(y)[:take].cpu().to(torch.long)
                    real_labels.append(y)
                    stats_r = score(stats_r, to_device_async(clips[:take], self.device).to(torch.float32), y)
                    n_real += take
                    if n_real >= n_samples:
                        break
            finally:
                torch.set_rng_state(rng_state)
            if n_real < n_samples:
                raise ValueError(f"`real` delivered {n_real} clips: n_samples={n_samples} are needed")
            n_classes = stats_r.n_classes
            out.update({"real_" + key: value for key, value in stats_r.result().items()})
            if labels is None:
                labels = self._check_labels(torch.cat(real_labels))
        if labels is None:
            labels = torch.arange(n_samples) % self.n_class
        if fidelity:
            if n_classes is None:
                side = 16 * self.G.latent_dim
                n_classes = classifier(torch.zeros(1, 3, self.n_frames, side, side, device=self.device)).shape[1]
            if int(labels.max()) >= n_classes:
                raise ValueError(f"fidelity=True: class id {int(labels.max())} has no logit among the classifier's {n_classes}; "
                                 "fidelity=False scores a classifier over another label set")
        stats = None
        with self._sampling_weights(use_ema, standing_stats), self._g_eval():
            for lo in range(0, n_samples, batch):
                y = labels[lo:lo + batch]
                z = self._draw_z(y.shape[0], truncation, gen)
                fake = self.G(to_device_async(z, self.device), to_device_async(y, self.device))
                stats = score(stats, fake.to(torch.float32).permute(0, 2, 1, 3, 4).contiguous(), y)
        out.update(stats.result(), n_classes=stats.n_classes)
        return out

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
        w, self._sheets = self._sheets, None
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
        with self._sampling_weights(self.sample_use_ema, None), self._g_eval() as put_back:
            for lo in range(0, n, chunk):
                raw = self.G(z[lo:lo + chunk], label[lo:lo + chunk])          # [b, T, 3, H, W] in [-1, 1]
                put_back()
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
        horizon, n_samples, frames, cond, labels_d, zs = self._prediction_inputs("save_predictions", clips, labels, horizon,
                                                                                  n_samples, seed)
        B, K_ = frames.shape[0], self.n_cond
        L_ = K_ + horizon
        ctx_view = frames[:, :K_]
        total = (1 + n_samples) * L_
        out = torch.empty((B,) + self._sheet_dims(total, frames, L_), dtype=torch.uint8, device=self.device)
        make_sheets(frames, nrow=L_, row_prefix=True, out=out, total_slots=total)                  # row 0, borders, every other slot
        with self._g_eval() as put_back:
            for s, raw in self._futures(cond, labels_d, horizon, zs, put_back):
                make_sheets(ctx_view, nrow=L_, row_prefix=True, out=out, first_slot=(1 + s) * L_, total_slots=total, fill=False)
                make_sheets(raw, nrow=L_, row_prefix=True, out=out, first_slot=(1 + s) * L_ + K_, total_slots=total, fill=False)
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
