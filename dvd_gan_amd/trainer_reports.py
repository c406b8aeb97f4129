"""What a Trainer reports about its run: the gradient guard's norms, the orthogonal penalty, the discriminators' logit statistics,
the consistency penalties and the singular values of the weights.  A plain base class of train_step.Trainer; nothing here is on the training step's path
but the device scalars the properties hand out, and each group has ONE call that synchronizes."""
from . import lib as L


class TrainerReports(object):
    @property
    def ortho_penalty(self):
        """Device scalar (float64): sum over the regularised matrices of 1/2 ||offdiag(W W^T)||_F^2, on the weights the last
        generator step started from, unscaled; None when config.g_ortho = 0 or before the first step."""
        return self.g_optimizer.ortho_penalty

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

    def cr_report(self):
        """The consistency penalties of the last D iteration as a host dict, or None when d_cr and d_cr_fake are both 0.  The one
        call of this group that synchronizes.  Per site (Ds_real, Ds_fake, Dt_real, Dt_fake): the penalty as it entered the
        network's loss, the mean squared gap between the logits of the transformed and of the clean views, the largest |gap|,
        the pairs whose gap is not zero, and the number of pairs n."""
        if self._cr_stats is None:
            return None
        s = self._cr_stats.cpu().tolist()
        return {site: {"penalty": row[L.CR_STAT_PENALTY], "mean_sq_gap": row[L.CR_STAT_MSQ], "max_abs_gap": row[L.CR_STAT_MAXABS],
                       "nonzero": int(row[L.CR_STAT_NONZERO]), "n": int(row[L.CR_STAT_N])}
                for site, row in zip(("Ds_real", "Ds_fake", "Dt_real", "Dt_fake"), s)}

    def zcr_report(self):
        """Latent consistency regularization of the last step as a host dict, or None when z_cr and z_cr_gen are both 0.  The one
        call of this group that synchronizes.  "Ds" / "Dt": the penalty of the last D iteration's fake call as it entered the
        network's loss, the mean squared gap between the logits of the base and of the partner clips, the largest |gap|, the pairs
        whose gap is not zero and the number of pairs n (cr_report()'s five fields).  "G": the term as it entered the generator's
        loss (-z_cr_gen * mean_sq_dist; zero while z_cr_gen = 0), the mean squared distance between base and partner clips, the
        smallest and the largest per-pair mean squared distance (min_pair: the pair the generator moved least), the largest
        |difference| of two elements, and the number of pairs."""
        if self._zcr_stats is None:
            return None
        s, g = self._zcr_stats.cpu().tolist(), self._zcr_stats_g.cpu().tolist()
        out = {tag: {"penalty": row[L.CR_STAT_PENALTY], "mean_sq_gap": row[L.CR_STAT_MSQ], "max_abs_gap": row[L.CR_STAT_MAXABS],
                     "nonzero": int(row[L.CR_STAT_NONZERO]), "n": int(row[L.CR_STAT_N])} for tag, row in zip(("Ds", "Dt"), s)}
        out["G"] = {"term": g[L.ZCR_STAT_TERM], "mean_sq_dist": g[L.ZCR_STAT_MSQ], "min_pair": g[L.ZCR_STAT_MIN_PAIR],
                    "max_pair": g[L.ZCR_STAT_MAX_PAIR], "max_abs_diff": g[L.ZCR_STAT_MAXABS], "pairs": int(g[L.ZCR_STAT_PAIRS])}
        return out

    # ---- singular values of the weights (spectral.py)
    def _sv_monitors(self):
        """One monitor per network over every trainable tensor with dim() >= 2 (named by its state_dict key), with the layer's
        weight_u / weight_v where it is spectrally normalised.  The ring's last row is sv_report()'s own."""
        if self._sv is None:
            from .spectral import SpectrumMonitor
            self._sv = {}
            for tag, net in self._nets():
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
                         # (an all-zero matrix -- a TSRU's flow head at initialisation -- has rank 0, not an undefined one)
                         "stable_rank": fro2[i] / sv[i][0] ** 2 if sv[i][0] > 0.0 else 0.0 if fro2[i] == 0.0 else float("nan"),
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
