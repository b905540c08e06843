"""Urban Radiance Fields' line-of-sight term on the weights along a ray, on the device.  ctypes binding of libraylos_hip.so
(include/raylos_hip.h).

A ray whose expected depth is right can still carry a floater half-way to the surface, balanced by weight behind it: the depth
losses on the expected depth see one number per ray, and kl rewards weight near the prior without penalising weight in front of
it.  `ray_los` puts one term on the foreground weights w [n, S] of one cascade level, with the ascending sample positions z [n, S],
the rays' far bounds [n], the depth prior p [n] (scene units, 0 = none) and the half-width sigma [n] of a band around it:

    supervised  p > 0 and p < far and sigma > 0
    w_s is the mass of the interval [z_s, z_{s+1}] (the last one ends at far)
    an interval that ends at or before p - sigma:        w_s^2                  the space in front of the band is emptied
    an interval that touches (p - sigma, p + sigma):     (w_s - k_s)^2          k_s = the mass of N(p, (sigma / 3)^2) in the interval
    an interval behind the band:                         nothing
    value = (1 / n) sum over the supervised rays

with gradients to the weights (positions, p and sigma receive none).  The definition is DESIGN.md 9.13 (restated as code in
tests/ray_los_reference.py).

One level per call, enqueued on torch's current stream; nothing synchronises.  torch only allocates.  There is no host path: without
libraylos_hip.so and a device `ray_los` raises.  The `check_*` helpers are the refusals of the trainer's keyword arguments and the
CLI's flags (ValueError); they need neither torch nor the library.
"""
import ctypes as C
import math
import numbers
import os

from . import _ctypes_util as U

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('RAYLOS_HIP_LIB') or os.path.join(_HERE, 'libraylos_hip.so')
OK = 0
ABI_VERSION = 1
MAX_RAYS = 1 << 20
MAX_SAMPLES = 1024

_fp = C.c_void_p
# every symbol include/raylos_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'raylos_last_error': (C.c_char_p, []),
    'raylos_abi_version': (C.c_int, []),
    'raylos_workspace_bytes': (C.c_int64, [C.c_int]),
    'raylos_level': (C.c_int, [_fp, C.c_int, C.c_int, _fp, _fp, _fp, _fp, _fp, C.c_double, _fp, _fp, _fp, _fp, _fp]),
}

_lib = None


class RayLosError(RuntimeError):
    pass


def lib():
    """The loaded library with typed prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        _lib = U.load(LIB_PATH, 'libraylos_hip.so', SYMBOLS, 'raylos_abi_version', ABI_VERSION, RayLosError,
                      ' (hipcc --offload-arch=gfx950). There is no CPU fallback for the line-of-sight term.')
    return _lib


def last_error():
    return lib().raylos_last_error().decode('utf-8', 'replace')


check = U.checker(lib, 'raylos_last_error', RayLosError, 'raylos call')


def workspace_bytes(n):
    """Size of the scratch buffer of a call; raises RayLosError for what the library rejects (n outside 1 .. 2^20).  Needs no GPU."""
    return U.size(lib().raylos_workspace_bytes(int(n)), last_error, RayLosError)


# a training run calls with one n per level, step after step: (device, n) -> the scratch buffer.  Calls of one stream are ordered, so
# the next call may overwrite it.
_workspaces = U.Workspaces(workspace_bytes, held=4)


# ------------------------------------------------------------------------------------------------ the flags
def _number(v, name):
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError('%s = %r: expected a number' % (name, v))
    return float(v)


def check_lambda(lam, name='lambda_los'):
    """The weight of the term: finite and not negative (0 = off), or ValueError.  Returns it as a float."""
    lam = _number(lam, name)
    if not math.isfinite(lam) or lam < 0.0:
        raise ValueError('%s = %r: expected a finite value that is not negative' % (name, lam))
    return lam


def check_sigma_source(los_sigma, los_sigma_std_mult):
    """The source of the band's half-width: los_sigma_std_mult > 0 takes that many standard deviations of the prior (the batch's
    depth_std), else los_sigma (metres) is the half-width and must be positive; ValueError for values that are not finite, for
    negative ones and for a missing source.  Returns (los_sigma as a float or None, los_sigma_std_mult as a float)."""
    mult = _number(los_sigma_std_mult, 'los_sigma_std_mult')
    if not math.isfinite(mult) or mult < 0.0:
        raise ValueError('los_sigma_std_mult = %r: expected a finite value that is not negative' % mult)
    if los_sigma is not None:
        los_sigma = _number(los_sigma, 'los_sigma')
        if not math.isfinite(los_sigma) or los_sigma < 0.0:
            raise ValueError('los_sigma = %r: expected a finite value in metres that is not negative' % los_sigma)
    if mult == 0.0 and not (los_sigma is not None and los_sigma > 0.0):
        raise ValueError('lambda_los: the band has no half-width: pass los_sigma (metres, positive), or los_sigma_std_mult (positive) '
                         "to take multiples of the prior's standard deviation")
    return los_sigma, mult


def check_min_sigma(min_sigma):
    min_sigma = _number(min_sigma, 'los_min_sigma')
    if not math.isfinite(min_sigma) or min_sigma < 0.0:
        raise ValueError('los_min_sigma = %r: expected a finite value in metres that is not negative' % min_sigma)
    return min_sigma


def check_decay(decay, steps):
    """URF's annealing of the band: the half-width is multiplied by decay ** (min(step, steps) / steps).  decay finite and positive,
    steps an integer that is not negative (0 = no annealing), or ValueError.  Returns (decay, steps)."""
    decay = _number(decay, 'los_sigma_decay')
    if not math.isfinite(decay) or decay <= 0.0:
        raise ValueError('los_sigma_decay = %r: expected a finite positive factor' % decay)
    if isinstance(steps, bool) or int(steps) != steps or int(steps) < 0:
        raise ValueError('los_sigma_decay_steps = %r: expected an integer that is not negative (0 = no annealing)' % (steps,))
    return decay, int(steps)


def check_combination(lambda_los, fuse_loss=False, use_depth=True, depth_loss_type='mse'):
    """What a positive lambda_los cannot be combined with, or ValueError"""
    if not lambda_los > 0:
        return
    if fuse_loss:
        raise ValueError('fuse_loss and lambda_los cannot be combined: the fused backward forms the loss gradient itself and '
                         'ignores g_fg_weights')
    if not use_depth:
        raise ValueError('lambda_los needs use_depth: the line-of-sight term is built around the depth prior of a ray')
    from . import depth_losses as DL
    row = DL.LOSSES.get(depth_loss_type)
    if row is not None and 'min_rays' in row.extra:       # the loss fits the prior's scale and shift batch by batch: a relative prior
        raise ValueError("lambda_los and depth_loss_type %r cannot be combined: a relative prior has no line of sight" % depth_loss_type)


def decay_factor(decay, steps, step):
    """decay ** (min(step, steps) / steps); 1 for steps = 0"""
    return 1.0 if steps == 0 else float(decay) ** (min(int(step), steps) / float(steps))


# ------------------------------------------------------------------------------------------------ the call
def _tensor(t, name, shape, dev):
    return U.inplace_f32(t, name, shape, dev, RayLosError, 'line-of-sight', 'weights')


def ray_los(weights, z, far, prior, sigma, lam, g_weights=None, fold_total=None):
    """The line-of-sight term of one level: weights [n, S], z [n, S] ascending sample positions, far [n] the rays' far bounds,
    prior [n] the depth prior in scene units (0 = none), sigma [n] the half-width of the band in scene units: float32 device
    tensors, n in 1 .. 2^20, S in 1 .. 1024.  A ray is supervised where prior > 0, prior < far and sigma > 0.  lam: finite and
    positive.  g_weights: a float32 device tensor [n, S] or None; lam * d value / d weights is ACCUMULATED, the row of an
    unsupervised ray keeps its bits.  fold_total: a one-element float32 device tensor or None, updated on the device after the
    value: fold_total += lam * value.
    Returns (values [1] = (the mean term), stats [2] = (supervised rays, their summed mass in front of the band)), float32 device
    tensors.  Enqueue only."""
    import torch
    if not isinstance(weights, torch.Tensor) or weights.dim() != 2:
        raise RayLosError('weights: expected a float32 device tensor [n, S], got %s' % (tuple(getattr(weights, 'shape', ())),))
    n, S = int(weights.shape[0]), int(weights.shape[1])
    if not 1 <= n <= MAX_RAYS:
        raise RayLosError('weights: %d rays, expected 1 .. 2^20 (the line-of-sight term is built for training batches)' % n)
    if not 1 <= S <= MAX_SAMPLES:
        raise RayLosError('weights: %d samples per ray, expected 1 .. %d' % (S, MAX_SAMPLES))
    dev = weights.device if weights.is_cuda else None
    _tensor(weights, 'weights', (n, S), dev)
    _tensor(z, 'z', (n, S), dev)
    _tensor(far, 'far', (n,), dev)
    _tensor(prior, 'prior', (n,), dev)
    _tensor(sigma, 'sigma', (n,), dev)
    if g_weights is not None:
        _tensor(g_weights, 'g_weights', (n, S), dev)
    if fold_total is not None:
        _tensor(fold_total, 'fold_total', tuple(getattr(fold_total, 'shape', ())), dev)
        if fold_total.numel() != 1:
            raise RayLosError('fold_total: expected a one-element float32 tensor, got shape %s' % (tuple(fold_total.shape),))
    lam = float(lam)
    if not math.isfinite(lam) or not lam > 0.0:
        raise RayLosError('lam = %r: expected a finite positive value' % lam)
    with torch.cuda.device(dev):
        ws = _workspaces.buffer(dev, n)
        out = torch.empty(3, device=dev)
        values, stats = out[:1], out[1:]
        check(lib().raylos_level(U.stream(), n, S, U.p(weights), U.p(z), U.p(far), U.p(prior), U.p(sigma), lam, U.p(g_weights),
                                 U.p(ws), U.p(values), U.p(stats), U.p(fold_total)), 'raylos_level')
    return values, stats
