"""The flag surface of the plane-sweep depth prior (depth_mvs.py): the parameters' names, defaults and help texts, and the adapters
that read them from a Config dict or from parsed flags.  Host side only and free of ctypes, so that a trainer can declare the flags
without importing the binding: depth_mvs and libdepthmvs_hip.so are loaded by a run that asks for the sweep."""
MAX_VIEWS, MIN_PLANES, MAX_PLANES, MAX_RADIUS = 16, 4, 256, 4
# the parameters: name -> (default, help).  near and far are in metres at both flag surfaces and in the units of the cameras at the call.
PARAMS = {
    'planes': (64, 'depth planes of the sweep, uniform in inverse depth between 1 / far and 1 / near (%d .. %d)' % (MIN_PLANES, MAX_PLANES)),
    'near': (2.0, 'depth of the nearest plane, in metres'),
    'far': (100.0, 'depth of the farthest plane, in metres (inf: the plane at infinity)'),
    'best_views': (0, 'views of a plane whose costs are summed, the best ones: the occlusion rule (1 .. views; 0 = half of them, rounded up)'),
    'agg_radius': (2, 'half width, in pixels, of the window the costs are aggregated over (0 .. %d)' % MAX_RADIUS),
    'uniqueness': (0.9, 'a pixel is accepted only where its best cost is at most this times the best cost more than one plane away (0 < u <= 1)'),
    'std_planes': (0.5, 'the standard deviation of an accepted pixel, in plane steps carried into depth'),
}
# the semi-global smoothing of the costs (depth_mvs_smooth.py): name -> (default, help).  They enter a call's parameters
# only when smooth_paths is not 0: without it the parameters, the call and what is loaded are those of the plain sweep.
SMOOTH = {
    'smooth_paths': (0, 'scanline directions the aggregated costs are summed along before the winner is taken: semi-global smoothing '
                        '(0 = off, 4 or 8)'),
    'smooth_p1': (1, 'penalty of a change of one plane between neighbouring pixels, per census bit of the aggregated cost (>= 1)'),
    'smooth_p2': (8, 'penalty of a jump of more than one plane, per census bit of the aggregated cost (>= smooth_p1)'),
    'smooth_edge': (0, 'luma step that halves smooth_p2 across an image edge: P2 / (1 + |dY| // smooth_edge), not below P1 '
                       '(0 = constant, 1 .. 255)'),
}
STD_FLOOR_HELP = 'lower bound, in metres, of the standard deviation the sweep writes for the gnll depth loss'
VIEWS_HELP = ('compute the depth prior of the training frames on the device when they are loaded, by a plane sweep of every frame against '
              'its N nearest frames; needs --depth_sup_type mvs, whose folder is then not read (0 = off; 1 .. %d)' % MAX_VIEWS)


def _scaled(p, scale):
    """near, far and std_floor: metres -> scene units"""
    for name in ('near', 'far', 'std_floor'):
        p[name] = float(p[name]) * float(scale)
    return p


def scene_params(cfg, scale=1.0):
    """The call's parameters of a Config dict (without views)"""
    p = {name: cfg.get('depth_mvs_' + name, default) for name, (default, _) in PARAMS.items()}
    p['std_floor'] = cfg.get('depth_mvs_std_floor', 0.0)
    if cfg.get('depth_mvs_smooth_paths', 0):
        p.update({name: cfg.get('depth_mvs_' + name, default) for name, (default, _) in SMOOTH.items()})
    return _scaled(p, scale)


def add_flags(parser, prefix='depth_mvs_'):
    """--depth_mvs_views, the parameters, the smoothing's and --depth_mvs_std_floor on an argparse parser (ddp_train_nerf); the CLI adds them
    without prefix, with its own --views"""
    if prefix:
        parser.add_argument('--%sviews' % prefix, type=int, default=0, help=VIEWS_HELP)
    for name, (default, text) in list(PARAMS.items()) + list(SMOOTH.items()):
        parser.add_argument('--%s%s' % (prefix, name), type=type(default), default=default, help='%s (default %s)' % (text, default))
    parser.add_argument('--%sstd_floor' % prefix, type=float, default=0.0, help='%s (default 0)' % STD_FLOOR_HELP)


def args_params(args, scale=1.0, prefix='depth_mvs_'):
    """The call's parameters of parsed flags (without views)"""
    p = {name: getattr(args, prefix + name) for name in PARAMS}
    p['std_floor'] = getattr(args, prefix + 'std_floor')
    if getattr(args, prefix + 'smooth_paths', 0):
        p.update({name: getattr(args, prefix + name) for name in SMOOTH})
    return _scaled(p, scale)
