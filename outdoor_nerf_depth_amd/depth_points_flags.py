"""The flag surface of the sparse-point depth prior (depth_points.py): the parameters' names, defaults and help texts, and the
adapters that read them from a Config dict or from parsed flags.  Host side only and free of ctypes, so that a trainer can declare
the flags without importing the binding: depth_points and libdepthpoints_hip.so are loaded by a run that asks for the stage."""
MAX_RADIUS = 8
MODES = ('track', 'all')
DEFAULT_RADIUS = {'track': 0, 'all': 4}
# the parameters: name -> (default, help).  near, far and std_floor are in metres at both flag surfaces and in the units of the
# cameras at the call; occl_radius -1 stands for the mode's default.
PARAMS = {
    'max_error': (2.0, 'a point is used only when its mean reprojection error is at most this, in pixels'),
    'min_track': (3, 'a point is used only when at least this many images of the model observe it'),
    'err_floor': (0.5, 'lower bound, in pixels, of the reprojection error that enters a point\'s standard deviation'),
    'near': (0.5, 'a point nearer to a frame than this, in metres, is not drawn into it'),
    'far': (200.0, 'a point farther from a frame than this, in metres, is not drawn into it'),
    'occl_radius': (-1, 'half width, in pixels, of the window in which a nearer point hides a farther one (0 .. %d; 0 = the pixel alone; '
                        '-1 = by mode: 0 for track, 4 for all)' % MAX_RADIUS),
    'occl_tol': (0.05, 'a point is hidden when it lies behind the nearest point of its window by more than this, relative to that point'),
    'std_scale': (1.0, 'factor on the standard deviation z^2 / (f B) * error that the stage writes for the gnll depth loss'),
    'std_floor': (0.0, 'lower bound, in metres, of that standard deviation'),
}
VIS_HELP = ('compute the depth prior (--depth_sup_type points) or the alignment\'s anchor (--depth_align_anchor points) of the training '
            'frames on the device when they are loaded, from the 3D points of the scene\'s reconstruction: track draws a point into the '
            'frames that observed it, all into every frame that holds it; the folder is then not read (empty = off)')
MODEL_HELP = ('the COLMAP model (cameras, images, points3D; .bin or .txt) whose 3D points become the depth prior (--depth_sup_type points) '
              'or the alignment\'s anchor (--depth_align_anchor points) of the training frames when they are loaded; the frames are matched '
              'to the model\'s images by file stem and the pose files must be a shifted, scaled copy of the model\'s cameras')


def _scaled(p, scale):
    """near, far and std_floor: metres -> scene units; occl_radius: -1 -> None (the mode's default)"""
    for name in ('near', 'far', 'std_floor'):
        p[name] = float(p[name]) * float(scale)
    if p['occl_radius'] is not None and int(p['occl_radius']) < 0:
        p['occl_radius'] = None
    return p


def scene_params(cfg, scale=1.0):
    """The parameters of a Config dict (without vis)"""
    return _scaled({name: cfg.get('depth_points_' + name, default) for name, (default, _) in PARAMS.items()}, scale)


def add_flags(parser, prefix='depth_points_'):
    """--depth_points_model, --depth_points_vis and the parameters on an argparse parser (ddp_train_nerf); the CLI adds the
    parameters without prefix, with its own --vis and --points_model"""
    if prefix:
        parser.add_argument('--%smodel' % prefix, default='', help=MODEL_HELP)
        parser.add_argument('--%svis' % prefix, default='track', choices=MODES, help='track: a point goes into the frames that observed '
                            'it; all: into every frame that holds it (default track)')
    for name, (default, text) in PARAMS.items():
        parser.add_argument('--%s%s' % (prefix, name), type=type(default), default=default, help='%s (default %s)' % (text, default))


def args_params(args, scale=1.0, prefix='depth_points_'):
    """The parameters of parsed flags (without vis)"""
    return _scaled({name: getattr(args, prefix + name) for name in PARAMS}, scale)
