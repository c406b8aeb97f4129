"""The optional fields of a Trainer's config: one row each, the ONE place that knows what an unset field means.

`SETTINGS` rows are (attribute of the Trainer, field of the config, cast, default): `Trainer.__init__` sets
`attribute = cast(getattr(config, field, default))` for every row in one loop, and the class carries `cast(default)` under the
same name (`DEFAULTS`), so a Trainer that never ran the constructor (`Trainer.__new__`, a subclass with an `__init__` of its
own) reads "off" wherever the constructor would have stored it.  What the fields mean is documented where they are checked
(`Trainer.__init__`) and in train_step.py's module docstring.  Required fields (adv_loss, z_dim, g_chn, ...) are not here: they are
plain reads that raise AttributeError.
"""
from .augment import parse_policy
from .geom_augment import parse_geom


def as_is(v):
    return v


def int_or_0(v):
    return int(v or 0)


def or_0(v):
    return v or 0


def or_none(v):
    return v or None


SETTINGS = (
    # frame-conditional prediction: context frames (0 = generation from noise)
    ("n_cond", "n_cond", int, 0),
    # the generator: optional attention blocks
    ("g_self_attn", "g_self_attn", as_is, False),
    ("g_sep_attn", "g_sep_attn", as_is, False),
    # generator weight average
    ("ema_decay", "ema_decay", float, 0.0),
    ("ema_start", "ema_start", int, 0),
    ("ema_standing_stats", "ema_standing_stats", int, 0),
    ("ema_stats_seed", "ema_stats_seed", int, 0),
    # orthogonal regularization
    ("g_ortho", "g_ortho", float, 0.0),
    # gradient guard
    ("g_clip_norm", "g_clip_norm", float, 0.0),
    ("d_clip_norm", "d_clip_norm", float, 0.0),
    ("skip_nonfinite", "skip_nonfinite", bool, False),
    ("grad_log", "grad_log", int, 0),
    # LeCam, top-k generator updates, logit statistics
    ("lecam", "lecam", float, 0.0),
    ("lecam_decay", "lecam_decay", float, 0.99),
    ("lecam_start", "lecam_start", int, 0),
    ("g_topk", "g_topk", float, 0.0),
    ("g_topk_decay", "g_topk_decay", float, 0.99),
    ("_d_stats_on", "d_stats", bool, False),
    # augmentation of the discriminators' inputs
    ("d_aug", "d_aug", parse_policy, ""),                   # (both parsers read an unset or empty value as "no group")
    ("d_aug_geom", "d_aug_geom", parse_geom, ""),
    ("d_aug_p", "d_aug_p", float, 1.0),
    ("d_aug_target", "d_aug_target", float, 0.0),
    ("d_aug_interval", "d_aug_interval", int, 4),
    ("d_aug_kimg", "d_aug_kimg", float, 500),
    ("d_aug_seed", "d_aug_seed", int, 0),
    # singular-value monitoring
    ("sv_log", "sv_log", int_or_0, 0),
    ("sv_iters", "sv_iters", int, 4),
    ("sv_log_rows", "sv_log_rows", int, 64),
    ("sv_k", "sv_k", int, 3),
    ("sv_block", "sv_block", int, 8),
    ("sv_seed", "sv_seed", int, 0),
    # schedule, reference-format checkpoints, logging
    ("lr_decay", "lr_decay", as_is, 0.9999),
    ("pretrained_model", "pretrained_model", as_is, None),
    ("model_save_epoch", "model_save_epoch", as_is, 0),
    ("log_epoch", "log_epoch", as_is, 1),
    # exact resume
    ("state_save_step", "state_save_step", int_or_0, 0),
    ("state_keep", "state_keep", int, 2),
    ("resume", "resume", or_none, None),
    # sample sheets
    ("sample_step", "sample_step", int_or_0, 0),
    ("sample_epoch", "sample_epoch", or_0, 0),
    ("test_batch_size", "test_batch_size", int, 8),
    ("sample_layout", "sample_layout", as_is, "frames"),
    ("sample_fps", "sample_fps", as_is, 8),
    ("sample_use_ema", "sample_use_ema", bool, False),
    ("sample_seed", "sample_seed", int, 0),
)

# {attribute: cast(default)}: what every row's attribute is when the config does not set its field
DEFAULTS = {attribute: cast(default) for attribute, _, cast, default in SETTINGS}
