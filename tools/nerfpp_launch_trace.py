#!/usr/bin/env python3
"""Does the NeRF++ training step of two checkouts put the same work on the same streams?  The check a refactor of trainer.py, ops.py
or render_single_image stands on; needs a GPU and both checkouts built.

    python tools/nerfpp_launch_trace.py <checkout>                  # print the trace
    python tools/nerfpp_launch_trace.py <checkout A> <checkout B>   # one child process per checkout; exit status 1 if they differ

Traced, in the order it happens:
  - every call through lib().<symbol> of _lib (nerfpp), ray_reg, ray_los, depth_guide, depth_ssi and depth_gnll, wrapped from their SYMBOLS as
    tools/mip360_launch_trace.py wraps mip360's: the symbol and its integer and float arguments, the fields of an argument struct one
    by one; a pointer prints as * or, when null, 0 -- never its value.  The stream argument (the first, where the headers
    under include/ name it `stream`) prints as main, update or level<m>, by comparison with the trainer's update_stream and
    level_streams;
  - torch.cuda.Event.record (the stream and a running ordinal), torch.cuda.Stream.wait_event (the waiting stream and the ordinal of the
    event's record line) and torch.Tensor.record_stream (the stream and the tensor's shape);
  - torch.rand, torch.zeros and torch.zeros_like, with the shape.
A section is a trainer and three consecutive train_steps at 64 rays, cascade (16, 32), split-bf16, on a synthetic batch with a 70 %
sparse prior; it ends, after flush() and one synchronise, with a SHA-256 over the bytes of every returned scalar tensor and every
level's gradients, parameters and Adam moments, so that two checkouts found identical have also computed the same bits.  Sections:
every depth loss; for mse and kl the overlap variants (no side streams, no concurrent backward, event taps, the fused loss head with
and without side streams); auto-exposure; the regularisers; depth-guided sampling on three kinds of batch; the three sources of the
uniforms; and render_single_image on two chunks, with and without guiding.
"""
import argparse
import ctypes as C
import functools
import glob
import hashlib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mip360_launch_trace import NUMBERS, compare, show, wrap              # noqa: E402

LIBS = ('_lib', 'ray_reg', 'ray_los', 'depth_guide', 'depth_ssi', 'depth_gnll')
N_RAYS, CASCADE, GUIDE = 64, (16, 32), 8
STREAMS = {}                        # stream handle -> label, of the section's trainer


def stream_label(handle):
    return STREAMS.get(handle, 'other') if handle else 'main'


def stream_first(checkout, symbols):
    """The symbols whose first parameter the checkout's headers name `stream`.  Only theirs prints as a stream label: a symbol that
    starts with a data pointer (nerfpp_rccl_comm_destroy today) prints it like any pointer"""
    text = ''.join(open(p).read() for p in sorted(glob.glob(os.path.join(checkout, 'include', '*.h'))))
    return {s for s in symbols if re.search(r'\b%s\(\s*void\s*\*\s*stream\b' % re.escape(s), text)}


def show_args(with_stream, name, argtypes, args):
    out = []
    for i, (t, v) in enumerate(zip(argtypes, args)):
        if i == 0 and name in with_stream:
            out.append(stream_label(v.value if isinstance(v, C.c_void_p) else v))
        elif isinstance(getattr(v, '_obj', None), C.Structure):           # C.byref(argument struct)
            out.append('{%s}' % ', '.join('%s=%s' % (f, show(ft, getattr(v._obj, f))) for f, ft in v._obj._fields_))
        elif isinstance(v, C.Array) and v._type_ in NUMBERS:
            out.append(repr(list(v)))
        else:
            out.append(show(t, v))
    return ', '.join(out)


def wrap_torch(torch, out):
    """the stream and event traffic and the torch launches of a step, written to `out` as they happen"""
    count = [0]
    label = lambda s: stream_label(s.cuda_stream)
    record, wait_event, record_stream = torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.Tensor.record_stream

    def traced_record(self, stream=None):
        count[0] += 1
        self._trace_ordinal = count[0]
        out.write('Event.record(%s) #%d\n' % (label(stream if stream is not None else torch.cuda.current_stream()), count[0]))
        return record(self) if stream is None else record(self, stream)

    def traced_wait_event(self, event):
        out.write('Stream.wait_event(%s, #%s)\n' % (label(self), getattr(event, '_trace_ordinal', '?')))
        return wait_event(self, event)

    def traced_record_stream(self, stream):
        out.write('Tensor.record_stream(%s, %s)\n' % (label(stream), tuple(self.shape)))
        return record_stream(self, stream)

    torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.Tensor.record_stream = traced_record, traced_wait_event, traced_record_stream
    for name in ('rand', 'zeros', 'zeros_like'):
        def traced(*a, _fn=getattr(torch, name), _name=name, **k):
            t = _fn(*a, **k)
            out.write('torch.%s(%s)\n' % (_name, tuple(t.shape)))
            return t
        setattr(torch, name, traced)


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def trace(checkout, out):
    sys.path.insert(0, os.path.abspath(checkout))
    import importlib
    import numpy as np
    import torch
    from outdoor_nerf_depth_amd.ddp_train_nerf import render_single_image
    from outdoor_nerf_depth_amd.model import init_level_params
    from outdoor_nerf_depth_amd.synthetic import SyntheticKitti
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    dev = torch.device('cuda:0')
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    for name in LIBS:
        try:
            M = importlib.import_module('outdoor_nerf_depth_amd.' + name)
        except ImportError:                                               # a checkout from before this library: its trace has no call of it
            continue
        with_stream = stream_first(checkout, M.SYMBOLS)
        assert with_stream, 'no symbol of %s takes a stream first: are the headers under %s/include?' % (name, checkout)
        wrap(M, out, functools.partial(show_args, with_stream))
    wrap_torch(torch, out)

    def batch(std=False, prior=True, frame=False):
        rs = np.random.RandomState(3)
        b = SyntheticKitti().random_batch(N_RAYS, rs)
        b['depth_sup'] = np.where(rs.rand(N_RAYS) < 0.7, rs.uniform(0.02, 0.2, N_RAYS), 0).astype(np.float32)
        if std:
            b['depth_std'] = (b['depth_sup'] * rs.uniform(0.01, 0.2, N_RAYS)).astype(np.float32)
        dropped = ('depth_gt',) if prior else ('depth_gt', 'depth_sup')
        t = {k: T(v) for k, v in b.items() if isinstance(v, np.ndarray) and k not in dropped}
        if frame:
            t['frame'] = 0
        return t

    def trainer(kw, concurrent=True):
        tr = NerfppTrainer(dev, precision=2, cascade_samples=CASCADE, level_params=init_level_params(len(CASCADE)), **kw)
        tr.concurrent_backward = concurrent
        STREAMS.clear()
        if tr.update_stream is not None:
            STREAMS[tr.update_stream.cuda_stream] = 'update'
            STREAMS.update({s.cuda_stream: 'level%d' % m for m, s in enumerate(tr.level_streams)})
        return tr

    def taps():
        ev = [{'fwd': tuple(torch.cuda.Event(enable_timing=True) for _ in range(2)),
               'bwd': tuple(torch.cuda.Event(enable_timing=True) for _ in range(4))} for _ in CASCADE]
        for e in ev:
            for x in e['fwd'] + e['bwd']:
                x.record()                                                # materialise the handles
        return ev

    def steps(name, kw, b, concurrent=True, tapped=False, uniforms=None, seed=None):
        out.write('==== %s\n' % name)
        tr = trainer(kw, concurrent)
        if seed is not None:
            torch.manual_seed(seed)
        scalars = []
        for i in range(3):
            out.write('-- step %d\n' % i)
            scalars += tr.train_step(b, uniforms=uniforms, events=taps() if tapped else None)
        tr.flush()
        torch.cuda.synchronize(dev)
        state = scalars + tr.grads + [e.params for e in tr.engines] + tr.exp_avg + tr.exp_avg_sq
        if tr.autoexpo is not None:
            state += [ae.params for ae in tr.autoexpo]
        out.write('sha256 %s\n' % digest(state))

    def render(name, kw):
        class Frame(object):                                              # what render_single_image reads of a ray sampler
            H, W = 8, N_RAYS // 8

            def get_all(self):
                b = SyntheticKitti().random_batch(N_RAYS, np.random.RandomState(3))
                return {k: b[k] for k in ('ray_o', 'ray_d', 'min_depth')}
        out.write('==== %s\n' % name)
        ret = render_single_image(0, 1, trainer(kw), Frame(), 48)         # two chunks: 48 and 16 rays
        torch.cuda.synchronize(dev)
        out.write('sha256 %s\n' % digest([v for level in ret for v in level.values()]))

    loss = lambda kind: dict(use_depth=False) if kind == 'rgbonly' else dict(use_depth=True, depth_loss_type=kind, lambda_depth=0.1)
    for kind in ('rgbonly', 'mse', 'l1', 'kl', 'ssi', 'gnll'):
        steps('loss %s' % kind, loss(kind), batch(std=kind == 'gnll'))
    for kind in ('mse', 'kl'):
        steps('%s, overlap_allreduce off' % kind, dict(loss(kind), overlap_allreduce=False), batch())
        steps('%s, concurrent_backward off' % kind, loss(kind), batch(), concurrent=False)
        steps('%s, event taps' % kind, loss(kind), batch(), tapped=True)
        steps('%s, fuse_loss' % kind, dict(loss(kind), fuse_loss=True), batch())
        steps('%s, fuse_loss, overlap_allreduce off' % kind, dict(loss(kind), fuse_loss=True, overlap_allreduce=False), batch())
    steps('auto-exposure', dict(loss('mse'), optim_autoexpo=True, img_names=['00/image_2/000000.png', '00/image_2/000001.png']),
          batch(frame=True))
    for kind in ('rgbonly', 'kl'):
        steps('regularisers, %s' % kind, dict(loss(kind), lambda_distortion=0.3, lambda_opacity=0.02), batch())
    guide = dict(loss('mse'), depth_guide_samples=GUIDE)
    steps('depth guide, prior with depth_std', guide, batch(std=True))
    steps('depth guide, prior with depth_guide_std', dict(guide, depth_guide_std=0.01), batch())
    steps('depth guide, no depth_sup', dict(loss('rgbonly'), depth_guide_samples=GUIDE), batch(prior=False))
    rs = np.random.RandomState(5)
    u = lambda S: T(rs.rand(N_RAYS, S))
    S0, S1 = CASCADE
    for name, kw, b, uni in (('uniforms', loss('mse'), batch(), dict(t_fg=u(S0), t_bg=u(S0), u_fg=u(S1), u_bg=u(S1))),
                             ('uniforms, depth guide', guide, batch(std=True),
                              dict(t_fg=u(S0), t_bg=u(S0), u_fg=u(S1 - GUIDE), u_bg=u(S1), v_fg=u(GUIDE)))):
        steps('%s: in-kernel RNG' % name, kw, b)
        steps('%s: torch_rng' % name, dict(kw, torch_rng=True), b, seed=0)
        steps('%s: replayed' % name, kw, b, uniforms=uni)
    render('render', loss('mse'))
    render('render, depth guide', guide)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('a')
    ap.add_argument('b', nargs='?')
    ap.add_argument('--show', type=int, default=40, help='print the first N lines of a unified diff where the traces differ')
    args = ap.parse_args()
    if args.b is None:
        trace(args.a, sys.stdout)
        return 0
    return compare(__file__, (args.a, args.b), args.show, per_section=True)


if __name__ == '__main__':
    sys.exit(main())
