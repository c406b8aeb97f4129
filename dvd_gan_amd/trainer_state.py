"""What a Trainer writes to and reads from disk: the full training state of exact resume (checkpoint.py; DESIGN section 8, "what
a step leaves for the next") and the reference-format, weights-only checkpoints (trainer.py:337-343 / 375-382).  A plain base
class of train_step.Trainer."""
import os

import torch

from . import dist as D
from . import settings as S


def _strip_module(sd):
    """The keys of a state_dict without nn.DataParallel's `module.` prefix."""
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


class TrainerState(object):
    def fingerprint(self):
        """The fields that decide shapes and arithmetic (checkpoint.FINGERPRINT): a state continues only a Trainer that agrees
        in all of them."""
        return {"g_chn": int(self.g_chn), "ds_chn": int(self.ds_chn), "dt_chn": int(self.dt_chn), "n_frames": int(self.n_frames),
                "n_cond": int(self.n_cond), "n_class": int(self.n_class), "z_dim": int(self.z_dim),
                "latent_dim": int(self.latent_dim), "g_self_attn": bool(self.g_self_attn),
                "g_sep_attn": bool(self.g_sep_attn), "compute_dtype": str(self.compute_dtype),
                "adv_loss": str(self.adv_loss), "d_iters": int(self.d_iters), "k_sample": int(self.k_sample),
                "batch_size": int(self.batch_size), "world_size": int(D.world_size()), "dp_mode": str(self.dp_mode)}

    def _resume_file(self):
        """config.resume -> the state file to continue from, or None (unset, or "latest" with no complete file yet)."""
        resume = self.resume
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
        if self.d_aug or self.d_aug_geom:
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
        world, keep = D.world_size(), self.state_keep
        os.makedirs(folder, exist_ok=True)
        own = self._host_state()
        if world > 1:
            C.atomic_save({"format_version": C.FORMAT_VERSION, "step": step, "rank": self.rank, "host": own},
                          C.state_path(folder, step, self.rank))
            if self.rank != 0:
                return
        host = {"step": step, "epoch": int(self._epoch), "opt": {}, "sched": {}, "rng": own["rng"],
                "loader": own["loader"], "frame_gen": None if self.frame_gen is None else self.frame_gen.get_state().clone()}
        if "aug" in own:
            host["aug"] = own["aug"]
        host["params"] = {tag: C.parameter_table(net) for tag, net in self._nets()}
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
        if self._anchors is not None:       # LeCam: both slots of each discriminator's anchors and the count
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
        w, self._state_writer = self._state_writer, None
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
        shape (trained ones included: a ConvGRU generator's state is refused by a TSRU generator, and vice versa, by name).
        In a data-parallel run every rank reads this file and its own `{step}_state.rank{r}.pt` next to it.  -> list of
        warning strings (settings that only steer future steps and differ from the file's; the constructor's hold)."""
        from . import checkpoint as C
        sd = C.load_file(path)
        C.check_fingerprint(sd["fingerprint"], self.fingerprint())
        tensors, host, step = sd["tensors"], sd["host"], int(sd["step"])
        for tag, net in self._nets():       # the trained tensors by name and shape, before anything is copied
            C.check_parameters(tag, host.get("params", {}).get(tag), net)
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
        if self._anchors is not None:
            saved = [tensors.get(f"lecam.{tag}") for tag in ("Ds", "Dt")]
            if any(t is None or tuple(t.shape) != (2, 2) for t in saved) or "lecam_it" not in host:
                self._anchors.zero_()
                self._lecam_it = 0
                notes.append("lecam: the state holds no anchors (it was written with lecam off): they start afresh")
            else:
                for net, t in enumerate(saved):
                    self._anchors[:, net].copy_(t)
                self._lecam_it = int(host["lecam_it"])
        if self.d_aug or self.d_aug_geom:
            saved = own.get("aug")
            if saved is None:                   # the LeCam anchors' rule: the constructor's p, a fresh generator, and a note
                self.d_aug_p = float(getattr(self.config, "d_aug_p", S.DEFAULTS["d_aug_p"]))
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

    # ---- trainer.py:337-343 / 375-382: reference-compatible checkpoints
    def save_models(self, step):
        """Rank 0 writes (its batch-norm running statistics are the ones saved in "replica" mode); the others wait.
        With a weight average (config.ema_decay > 0) a fourth file `{step}_G_ema.pth` holds G.state_dict() taken inside
        ema_weights(standing_stats=config.ema_standing_stats): the keys of `{step}_G.pth`, loadable into a plain Generator.  A
        frame-conditional Trainer has no context frames at this point: its file carries the averaged weights with the LIVE
        running statistics whatever ema_standing_stats says.  In a data-parallel run every rank enters the block and runs
        the standing-statistics passes (same seed: cross-replica collectives pair up); rank 0 writes."""
        writer = self._is_writer()
        if writer:
            os.makedirs(self.model_save_path, exist_ok=True)
            for tag, net in self._nets():
                torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()},
                           os.path.join(self.model_save_path, "{}_{}.pth".format(step, tag)))
        if self._ema_on():
            n_pass = 0 if self.n_cond else self.ema_standing_stats
            with self.ema_weights(standing_stats=n_pass):
                if writer:
                    torch.save({k: v.detach().cpu() for k, v in self.G.state_dict().items()},
                               os.path.join(self.model_save_path, "{}_G_ema.pth".format(step)))
        if D.world_size() > 1:
            torch.distributed.barrier()

    def load_pretrained_model(self):
        for tag, net in self._nets():
            sd = torch.load(os.path.join(self.model_save_path, "{}_{}.pth".format(self.pretrained_model, tag)),
                            map_location="cpu")
            net.load_state_dict(_strip_module(sd))          # DataParallel prefix
        # the average: its own file when there is one, else it starts from the weights just loaded (FlatAdam copies them at
        # the first step)
        path = os.path.join(self.model_save_path, "{}_G_ema.pth".format(self.pretrained_model))
        if self._ema_on() and os.path.exists(path):
            sd = _strip_module(torch.load(path, map_location="cpu"))
            flat = torch.cat([sd[k].reshape(-1).float() for k, p in self.G.named_parameters() if p.requires_grad])
            self.g_optimizer.load_ema(flat.to(self.g_optimizer.flat.device))
