"""Every depth loss of both training paths: one table, and the one call that runs the losses which are not part of a core loss head.

A depth loss is either a code of a path's core head (nerfpp_loss: _lib.LOSS_TYPES; mip360_losses: mip360.DEPTH_TYPES) or an
AFTER-call: the head runs without a depth term, and `after` then adds the loss of every level in one call of its own library --
value, gradients (accumulated onto the head's buffers) and the fold into the head's scalars, all on the device.  Adding a loss of
that kind: DESIGN.md 9.10.

Plain data, importable without torch and without any binding: a binding module is imported by the first call that needs it.
"""
import collections

AFTER = 'after'
# nerfpp / mip360: the loss on that path -- an int (the core head's code), AFTER, or None (not accepted there)
# inputs:  the per-ray inputs a training step must carry beside depth_sup ('depth_std'; 'cam_idx' where a batch mixes frames)
# refuses: the NerfppTrainer options the loss cannot be combined with (REFUSAL says why)
# log:     (name, numerator column, denominator column) of the log tail, columns of the last level's stats row
# stats:   the trainer attribute the stats of a step are left in (where the trainer has it)
# call / reads / extra: an AFTER loss's adapter below, the per-level lists it reads and the keys of `extra` it takes
# missing: what mip360.losses() says when one of those is not given
Loss = collections.namedtuple('Loss', 'nerfpp mip360 inputs refuses log stats call reads extra missing',
                              defaults=(None, None, (), (), None, None, None, (), (), None))


def _kl_ray(levels, prior, scale, grads, fold, extra):
    from . import mip360
    return mip360.depth_loss_rays('kl_ray', levels['weights'], levels['x'], prior, None, extra['directions'], extra['sigma'], scale,
                                  grads['weights'], None, extra['scalars']), None


def _urf_ray(levels, prior, scale, grads, fold, extra):
    from . import mip360
    return mip360.depth_loss_rays('urf_ray', levels['weights'], levels['x'], prior, levels['pred'], None, extra['sigma'], scale,
                                  grads['weights'], grads['pred'], extra['scalars']), None


def _ssi(levels, prior, scale, grads, fold, extra):
    from . import depth_ssi
    result = depth_ssi.ssi_loss(levels['pred'], prior, extra.get('group'), extra.get('n_groups', 1),
                                extra.get('min_rays', depth_ssi.DEFAULT_MIN_RAYS), extra.get('norm', 'all'), scale, grads['pred'], fold)
    return result, result[2]


def _gnll(levels, prior, scale, grads, fold, extra):
    from . import depth_gnll
    result = depth_gnll.gnll_loss(levels['weights'], levels['x'], levels['pred'], prior, extra['prior_std'], extra.get('limit'),
                                  extra.get('edges', False), scale, grads['weights'], grads['pred'], fold)
    return result, result[1]


_AFTER_REFUSES = ('fuse_loss', 'optim_autoexpo')          # the head runs rgb-only: neither can see the depth term
LOSSES = collections.OrderedDict([
    ('rgbonly', Loss(nerfpp=0)),                          # (NerfppTrainer(use_depth=False); no name of a depth loss)
    (None, Loss(mip360=0)),
    ('none', Loss(mip360=0)),
    ('mse', Loss(nerfpp=1, mip360=1)),
    ('l1', Loss(nerfpp=2, mip360=2)),
    ('kl', Loss(nerfpp=3, mip360=3)),                     # mip360: upstream's per-level reduction, depth_loss_klurf
    ('urf', Loss(mip360=4)),                              # the same
    ('kl_ray', Loss(mip360=AFTER, call=_kl_ray, reads=('weights', 'x'), extra=('directions', 'sigma', 'scalars'))),
    ('urf_ray', Loss(mip360=AFTER, call=_urf_ray, reads=('weights', 'x', 'pred'), extra=('sigma', 'scalars'))),
    ('ssi', Loss(nerfpp=AFTER, mip360=AFTER, inputs=('cam_idx',), refuses=_AFTER_REFUSES, log=('ssi_fit', 1, 0), stats='last_ssi_stats',
                 call=_ssi, reads=('pred',), extra=('group', 'n_groups', 'min_rays', 'norm'),
                 missing="depth_loss_type 'ssi' needs the proposal levels' distance_mean (dm_prop) and ssi = dict(group=, n_groups=, "
                         "min_rays=)")),
    ('gnll', Loss(nerfpp=AFTER, mip360=AFTER, inputs=('depth_std',), refuses=_AFTER_REFUSES, log=('gnll_gated', 1, 0),
                  stats='last_gnll_stats', call=_gnll, reads=('weights', 'x', 'pred'), extra=('prior_std', 'limit', 'edges'),
                  missing="depth_loss_type 'gnll' needs tdist_nerf, tdist_prop, the proposal levels' distance_mean (dm_prop) and "
                          "gnll = dict(prior_std=): the standard deviation of the prior, per ray")),
])
DEAD = ('los', 'nll')                                     # names of the reference's CLI whose code is dead there: refused
REFUSAL = {'fuse_loss': 'the fused compositing backward forms the depth gradient itself, from mse / l1 / kl only',
           'optim_autoexpo': "the auto-exposure gradient is taken from the loss head's own depth term"}
INPUTS = {'depth_std': 'the standard deviation of the prior', 'cam_idx': "the rays' frame indices"}


def names(path, kind=None):
    """The names the path ('nerfpp' / 'mip360') accepts, in table order; kind=AFTER: only those that run as an after-call"""
    return tuple(n for n, row in LOSSES.items() if getattr(row, path) is not None and kind in (None, getattr(row, path)))


def needs(name, what):
    """Does a step of the loss `name` (any name: an unknown one needs nothing) have to carry the per-ray input `what`?"""
    row = LOSSES.get(name)
    return row is not None and what in row.inputs


def after(kind, levels, prior, scale, grads, fold, extra):
    """The AFTER loss `kind` of all levels in one call.  levels / grads: {'weights' | 'x' | 'pred': one tensor per level} (the lists
    LOSSES[kind].reads names / the buffers their gradients are accumulated in), prior [n], scale: the levels' weights, fold: the
    head's scalars to update (ssi_loss's `fold`), extra: LOSSES[kind].extra.  Returns (what the binding returned, stats or None)."""
    return LOSSES[kind].call(levels, prior, scale, grads, fold, extra)


def kept_stats(trainer, loss_type):
    """The stats of the last step's depth loss where the trainer keeps them (LOSSES[...].stats), else None"""
    row = LOSSES.get(loss_type)
    return getattr(trainer, row.stats, None) if row is not None and row.stats is not None else None


def depth_log_tail(loss_type, stats):
    """' name=share' for a training log line from the per-level stats a trainer kept of its last step, '' where there is none"""
    row = LOSSES.get(loss_type)
    if row is None or row.log is None or stats is None:
        return ''
    name, num, den = row.log
    s = stats[-1].reshape(-1).cpu().numpy()
    return ' %s=%.3f' % (name, s[num] / max(s[den], 1.0))
