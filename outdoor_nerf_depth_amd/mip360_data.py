"""Scene reader and configuration of the MipNeRF-360 front end (nerf-methods/mipnerf360, configs/360.gin on the paper's
KITTI "DTU_format" scenes).

Mirrors `datasets.LLFF._load_renderings` (internal/datasets.py:560-761) for the path 360.gin takes: a COLMAP model (not
forward-facing, not raw), poses as `NeRFSceneManager.process` (:62-150) makes them, `camera_utils.transform_poses_pca`
(camera_utils.py:191-227), KITTI 16-bit depth PNGs, and the train / test split.  The COLMAP reader is written from the
file-format definition (binary and text models: cameras, images); pycolmap is not needed.  Decode and file I/O stay on the
host; `Scene.device_frames` puts a split's frames on the device once (rgb uint8, depths float32) for
`mip360.sample_batch` / `mip360.frame_rays`.

The configuration is the reference scripts' flag surface: `--gin_configs <file>` and repeated
`--gin_bindings "Config.key = value"` (scripts/train_kitti.sh, eval_kitti.sh).  `parse_gin` reads the Config keys this
front end honours (defaults = configs/360.gin on top of internal/configs.py) and accepts model bindings only where they
equal what the HIP kernels implement (360.gin's), plus the per-image appearance embeddings of configs/360_glo4.gin
(`Model.num_glo_features` 0..4, `Model.num_glo_embeddings`); anything else is an error that names the binding.
"""
import ast
import os
import struct

import numpy as np

from . import depth_losses as DL
from . import depth_prior_stages as PS

# ------------------------------------------------------------------------------------------------------------ config
# internal/configs.py defaults with configs/360.gin applied on top (dataset_loader, near, far, batch_size,
# compute_disp_metrics, auto_adjust_near_far)
CONFIG_DEFAULTS = dict(
    dataset_loader='llff', data_dir=None, checkpoint_dir=None, max_steps=250000, batch_size=4096, sample_every=1, factor=0,
    llffhold=8, load_alphabetical=True, near=0.2, far=1e6, auto_adjust_near_far=True, depth_loss_type='mse',
    depth_sup_type='gt', lambda_depth=0.1, depth_sigma=0.01, depth_ssi_min_rays=8, depth_gnll_std=0.0, depth_crop_range=0.0, depth_keep_ratio=0.0,
    compute_disp_metrics=True, checkpoint_every=25000, print_every=100, eval_suffix='', eval_quantize_metrics=True,
    render_chunk_size=16384, lr_init=0.002, lr_final=0.00002, lr_delay_steps=512, lr_delay_mult=0.01,
    # The stages that compute or repair the training split's prior when it goes to the device, all off by default; they run in the
    # order of depth_prior_stages.STAGES.  Lengths (near, far, max_depth, std_floor) are in metres.
    # the multi-view consistency check (depth_consistency.py; 0 views = off)
    depth_cons_views=0, depth_cons_min_views=2, depth_cons_pix_tol=1.0, depth_cons_rel_tol=0.01, depth_cons_keep_unverified=True,
    depth_cons_std_floor=0.0,
    # the accumulation of the neighbouring frames' prior into every training frame's (depth_accumulate.py; 0 views = off)
    depth_acc_views=0, depth_acc_occl_radius=2, depth_acc_occl_tol=0.05,
    # the alignment of the (relative) prior to the metric prior of type depth_align_anchor (depth_align.py; '' = off)
    depth_align_anchor='', depth_align_space='depth', depth_align_iters=10, depth_align_c=1.0, depth_align_min_points=16,
    depth_align_max_depth=float('inf'), depth_align_keep_anchor=False,
    # the completion of the prior under each frame's own image (depth_complete.py; 0 passes = off)
    depth_comp_iters=0, depth_comp_radius=4, depth_comp_sigma_space=2.0, depth_comp_sigma_colour=20.0, depth_comp_min_conf=0.02,
    depth_comp_min_points=2, depth_comp_max_rel_spread=0.1, depth_comp_decay=0.5, depth_comp_std_floor=0.0,
    # the plane sweep that computes the prior from the split's own images and cameras (depth_mvs.py; 0 views = off; needs
    # depth_sup_type = 'mvs', whose folder is then not read)
    depth_mvs_views=0, depth_mvs_planes=64, depth_mvs_near=2.0, depth_mvs_far=100.0, depth_mvs_best_views=0, depth_mvs_agg_radius=2,
    depth_mvs_uniqueness=0.9, depth_mvs_std_planes=0.5, depth_mvs_std_floor=0.0,
    # ... with semi-global smoothing of its costs along 4 or 8 scanline directions (depth_mvs_smooth.py; 0 paths = off)
    depth_mvs_smooth_paths=0, depth_mvs_smooth_p1=1, depth_mvs_smooth_p2=8, depth_mvs_smooth_edge=0,
    # the splat of the reconstruction's 3D points that computes the prior (depth_sup_type = 'points') or the alignment's anchor
    # (depth_align_anchor = 'points'; depth_points.py; '' = off, 'track' or 'all'; the folder is then not read); occl_radius -1 = by mode
    depth_points_vis='', depth_points_max_error=2.0, depth_points_min_track=3, depth_points_err_floor=0.5, depth_points_near=0.5,
    depth_points_far=200.0, depth_points_occl_radius=-1, depth_points_occl_tol=0.05, depth_points_std_scale=1.0,
    depth_points_std_floor=0.0)

# The model bindings of configs/360.gin: the network / sampler shape the kernels of libmip360_hip.so are built for.
MODEL_BINDINGS = {
    'Model.raydist_fn': '@jnp.reciprocal', 'Model.opaque_background': True,
    'PropMLP.warp_fn': '@coord.contract', 'PropMLP.net_depth': 4, 'PropMLP.net_width': 256,
    'PropMLP.disable_density_normals': True, 'PropMLP.disable_rgb': True,
    'NerfMLP.warp_fn': '@coord.contract', 'NerfMLP.net_depth': 8, 'NerfMLP.net_width': 1024,
    'NerfMLP.disable_density_normals': True,
}
# Model bindings with a range: per-image appearance embeddings (internal/models.py:64-65; configs/360_glo4.gin binds
# num_glo_features = 4).  The Config dict carries them under the same names; 0 features = the model of configs/360.gin.
MODEL_DEFAULTS = dict(num_glo_features=0, num_glo_embeddings=1000)
MAX_GLO_FEATURES = 4


class ConfigError(ValueError):
    pass


def _glo_binding(cfg, key, val, where):
    is_int = isinstance(val, int) and not isinstance(val, bool)
    if key == 'Model.num_glo_features':
        if not is_int or not 0 <= val <= MAX_GLO_FEATURES:
            raise ConfigError("%s: binding %s = %r is not supported: an integer in 0..%d.  The embedding rides in the zero padding of "
                              "the view layer's input row (256 bottleneck + 27 direction features, padded to 288 columns for the "
                              "matrix cores): columns 283..286 take up to %d features and column 287 stays the guaranteed-zero K "
                              "padding" % (where, key, val, MAX_GLO_FEATURES, MAX_GLO_FEATURES))
    elif not is_int or val < 1:
        raise ConfigError('%s: binding %s = %r is not supported: a positive integer' % (where, key, val))
    cfg[key[len('Model.'):]] = val


def check_glo_frames(cfg, n_train_frames):
    """train.py:82-84: with embeddings, every training frame needs a row of its own"""
    if int(cfg['num_glo_features']) > 0 and int(n_train_frames) > int(cfg['num_glo_embeddings']):
        raise ConfigError('Number of training images (%d) exceeds Model.num_glo_embeddings = %d with Model.num_glo_features = %d: '
                          'raise Model.num_glo_embeddings' % (n_train_frames, cfg['num_glo_embeddings'], cfg['num_glo_features']))


def _value(text, where):
    text = text.strip()
    if text.startswith('@'):
        return text
    try:
        return ast.literal_eval(text)
    except (ValueError, SyntaxError):
        raise ConfigError('%s: cannot parse the value %r' % (where, text))


def _apply(cfg, line, where):
    if '=' not in line:
        raise ConfigError('%s: expected `Scope.key = value`, got %r' % (where, line))
    key, val = line.split('=', 1)
    key = key.strip()
    val = _value(val, where)
    if key.startswith('Config.'):
        name = key[len('Config.'):]
        if name not in CONFIG_DEFAULTS:
            raise ConfigError('%s: binding %r is not a Config key this front end honours (%s)'
                              % (where, key, ', '.join(sorted(CONFIG_DEFAULTS))))
        if name == 'dataset_loader' and val != 'llff':
            raise ConfigError("%s: binding %s = %r: only the 'llff' (COLMAP) loader is implemented" % (where, key, val))
        cfg[name] = val
        return
    if key in MODEL_BINDINGS and MODEL_BINDINGS[key] == val:
        return
    if key in ('Model.num_glo_features', 'Model.num_glo_embeddings'):
        return _glo_binding(cfg, key, val, where)
    raise ConfigError('%s: binding %s = %r is not supported: the model is fixed to configs/360.gin (%s), with Model.num_glo_features '
                      'in 0..%d and Model.num_glo_embeddings free' % (where, key, val, ', '.join('%s = %r' % kv for kv in MODEL_BINDINGS.items()),
                                                                      MAX_GLO_FEATURES))


def strip_comment(line):
    """`line` without its `#` comment; a `#` inside a quoted string is kept."""
    quote = None
    for i, ch in enumerate(line):
        if quote:
            if ch == '\\':
                continue
            if ch == quote and line[i - 1] != '\\':
                quote = None
        elif ch in ('"', "'"):
            quote = ch
        elif ch == '#':
            return line[:i]
    return line


def parse_gin(config_files=(), bindings=()):
    """The gin subset the reference scripts use: `Scope.key = value` lines (python literals, `@name` references,
    `#` comments) from every config file, then the bindings in order.  Returns the Config dict."""
    cfg = dict(CONFIG_DEFAULTS, **MODEL_DEFAULTS)
    for path in config_files or ():
        with open(path) as f:
            for no, raw in enumerate(f, 1):
                line = strip_comment(raw).strip()
                if line:
                    _apply(cfg, line, '%s:%d' % (path, no))
    for b in bindings or ():
        for line in b.split('\n'):
            line = strip_comment(line).strip()
            if line:
                _apply(cfg, line, '--gin_bindings')
    return cfg


def add_gin_flags(parser):
    parser.add_argument('--gin_configs', action='append', default=[], help='gin config file (e.g. configs/360.gin)')
    parser.add_argument('--gin_bindings', action='append', default=[], help='"Config.key = value"')
    parser.add_argument('--logtostderr', action='store_true', help='accepted for compatibility (logs go to stdout)')


# ------------------------------------------------------------------------------------------------------- COLMAP model
# model id -> (name, number of parameters), from COLMAP's camera model list
CAMERA_MODELS = {0: ('SIMPLE_PINHOLE', 3), 1: ('PINHOLE', 4), 2: ('SIMPLE_RADIAL', 4), 3: ('RADIAL', 5), 4: ('OPENCV', 8),
                 5: ('OPENCV_FISHEYE', 8), 6: ('FULL_OPENCV', 12), 7: ('FOV', 5), 8: ('SIMPLE_RADIAL_FISHEYE', 4),
                 9: ('RADIAL_FISHEYE', 5), 10: ('THIN_PRISM_FISHEYE', 12)}
MODEL_IDS = {name: i for i, (name, _) in CAMERA_MODELS.items()}


def _read(f, fmt):
    n = struct.calcsize(fmt)
    data = f.read(n)
    if len(data) != n:
        raise ValueError('truncated COLMAP file')
    return struct.unpack(fmt, data)


def read_cameras_bin(path):
    """{camera_id: (model name, width, height, params)}"""
    cams = {}
    with open(path, 'rb') as f:
        (count,) = _read(f, '<Q')
        for _ in range(count):
            cid, mid, w, h = _read(f, '<iiQQ')
            if mid not in CAMERA_MODELS:
                raise ValueError('%s: unknown camera model id %d' % (path, mid))
            name, npar = CAMERA_MODELS[mid]
            cams[cid] = (name, int(w), int(h), np.array(_read(f, '<%dd' % npar)))
    return cams


def read_images_bin(path):
    """{image_id: (qvec (w, x, y, z), tvec, camera_id, name)} in file order"""
    images = {}
    with open(path, 'rb') as f:
        (count,) = _read(f, '<Q')
        for _ in range(count):
            iid, qw, qx, qy, qz, tx, ty, tz, cid = _read(f, '<idddddddi')
            name = b''
            while True:
                c = f.read(1)
                if c in (b'\x00', b''):
                    break
                name += c
            (npts,) = _read(f, '<Q')
            f.seek(24 * npts, 1)                      # (x, y, point3D id) per 2D point: not needed
            images[iid] = (np.array([qw, qx, qy, qz]), np.array([tx, ty, tz]), cid, name.decode('utf-8'))
    return images


def _data_lines(path):
    with open(path) as f:
        return [l.rstrip('\n') for l in f if not l.startswith('#')]


def read_cameras_txt(path):
    cams = {}
    for line in _data_lines(path):
        tok = line.split()
        if not tok:
            continue
        name = tok[1]
        if name not in MODEL_IDS:
            raise ValueError('%s: unknown camera model %s' % (path, name))
        cams[int(tok[0])] = (name, int(tok[2]), int(tok[3]), np.array([float(v) for v in tok[4:]]))
    return cams


def read_images_txt(path):
    images = {}
    lines = _data_lines(path)
    i = 0
    while i < len(lines):
        tok = lines[i].split()
        if not tok:                                   # (a blank line may stand where an image has no 2D points)
            i += 1
            continue
        iid = int(tok[0])
        q = np.array([float(v) for v in tok[1:5]])
        t = np.array([float(v) for v in tok[5:8]])
        images[iid] = (q, t, int(tok[8]), ' '.join(tok[9:]))
        i += 2                                        # the next line holds the image's 2D points
    return images


def _points3d(path, xyz, error, lengths, image_id):
    """(xyz float64 [P, 3], error float64 [P], off int64 [P + 1], image_id int32 [T]) of what a points3D reader collected"""
    if not xyz:
        raise ValueError('%s holds no 3D point (a reconstruction from known poses that was never triangulated writes such a file)' % path)
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(np.asarray(lengths, np.int64), out=off[1:])
    return (np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(error, np.float64), off,
            np.concatenate(image_id).astype(np.int32) if image_id else np.zeros(0, np.int32))


def read_points3d_bin(path):
    """The 3D points of a COLMAP model: (xyz float64 [P, 3], error float64 [P] (mean reprojection error, pixels), off int64 [P + 1],
    image_id int32 [T]): the track of point p is image_id[off[p]:off[p + 1]] (COLMAP image ids; the 2D point indices are dropped)"""
    xyz, error, lengths, image_id = [], [], [], []
    with open(path, 'rb') as f:
        try:
            (count,) = _read(f, '<Q')
            for _ in range(count):
                _, x, y, z, _, _, _, err, n = _read(f, '<QdddBBBdQ')
                data = f.read(8 * n)                                 # (image id, 2D point index) int32 pairs
                if len(data) != 8 * n:
                    raise ValueError('truncated COLMAP file')
                xyz.append((x, y, z))
                error.append(err)
                lengths.append(n)
                image_id.append(np.frombuffer(data, '<i4').reshape(-1, 2)[:, 0])
        except ValueError:
            raise ValueError('%s is truncated: it ends before point %d is complete' % (path, len(xyz))) from None
    return _points3d(path, xyz, error, lengths, image_id)


def read_points3d_txt(path):
    """read_points3d_bin of the text form: POINT3D_ID X Y Z R G B ERROR then (IMAGE_ID POINT2D_IDX) pairs, one point per line"""
    xyz, error, lengths, image_id = [], [], [], []
    for no, line in enumerate(_data_lines(path)):
        tok = line.split()
        if not tok:
            continue
        if len(tok) < 8 or (len(tok) - 8) % 2:
            raise ValueError('%s is truncated: data line %d has %d fields, expected 8 and then pairs' % (path, no + 1, len(tok)))
        xyz.append([float(v) for v in tok[1:4]])
        error.append(float(tok[7]))
        lengths.append((len(tok) - 8) // 2)
        image_id.append(np.array([int(v) for v in tok[8::2]], np.int64))
    return _points3d(path, xyz, error, lengths, image_id)


def read_points3d(sparse_dir):
    """The 3D points of a COLMAP model directory (binary preferred, text otherwise)"""
    if os.path.exists(os.path.join(sparse_dir, 'points3D.bin')):
        return read_points3d_bin(os.path.join(sparse_dir, 'points3D.bin'))
    if os.path.exists(os.path.join(sparse_dir, 'points3D.txt')):
        return read_points3d_txt(os.path.join(sparse_dir, 'points3D.txt'))
    raise FileNotFoundError('no 3D points (points3D.bin / points3D.txt) in %s' % sparse_dir)


def read_model(sparse_dir):
    """cameras, images of a COLMAP model directory (binary preferred, text otherwise)."""
    if os.path.exists(os.path.join(sparse_dir, 'cameras.bin')):
        return read_cameras_bin(os.path.join(sparse_dir, 'cameras.bin')), read_images_bin(os.path.join(sparse_dir, 'images.bin'))
    if os.path.exists(os.path.join(sparse_dir, 'cameras.txt')):
        return read_cameras_txt(os.path.join(sparse_dir, 'cameras.txt')), read_images_txt(os.path.join(sparse_dir, 'images.txt'))
    raise FileNotFoundError('no COLMAP model (cameras.bin / cameras.txt) in %s' % sparse_dir)


def camera_model_name(sparse_dir):
    """The COLMAP model name of camera 1 (the camera every image shares), e.g. 'PINHOLE' or 'OPENCV'"""
    binary = os.path.join(sparse_dir, 'cameras.bin')
    cams = read_cameras_bin(binary) if os.path.exists(binary) else read_cameras_txt(os.path.join(sparse_dir, 'cameras.txt'))
    return cams[1][0]


def qvec_to_rotmat(q):
    """Rotation matrix of a unit quaternion (w, x, y, z), COLMAP's convention (world-to-camera rotation)."""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def camera_intrinsics(model, params):
    """(fx, fy, cx, cy, distortion dict or None) of a COLMAP camera, with NeRFSceneManager.process's distortion keys."""
    p = list(params)
    if model == 'SIMPLE_PINHOLE':
        return p[0], p[0], p[1], p[2], None
    if model == 'PINHOLE':
        return p[0], p[1], p[2], p[3], None
    if model == 'SIMPLE_RADIAL':
        return p[0], p[0], p[1], p[2], dict(k1=p[3], k2=0., k3=0., p1=0., p2=0.)
    if model == 'RADIAL':
        return p[0], p[0], p[1], p[2], dict(k1=p[3], k2=p[4], k3=0., p1=0., p2=0.)
    if model == 'OPENCV':
        return p[0], p[1], p[2], p[3], dict(k1=p[4], k2=p[5], k3=0., p1=p[6], p2=p[7])
    if model == 'OPENCV_FISHEYE':
        raise ValueError('camera model OPENCV_FISHEYE: fisheye projection is not supported by this front end '
                         '(perspective models only: SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV)')
    raise ValueError('camera model %s is not supported (SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV)' % model)


def load_colmap_poses(sparse_dir, load_alphabetical=True):
    """NeRFSceneManager.process (datasets.py:62-150) + the alphabetical sort (:590-595): image names, camera-to-world poses
    [N, 3, 4] in the NeRF frame (right, up, back), pixtocam [3, 3] of camera 1, distortion dict or None."""
    cams, images = read_model(sparse_dir)
    if 1 not in cams:
        raise ValueError('%s: camera 1 missing (intrinsics are taken from camera 1, shared by all images)' % sparse_dir)
    fx, fy, cx, cy, dist = camera_intrinsics(cams[1][0], cams[1][3])
    pixtocam = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.]]))
    names, poses = [], []
    for iid in images:
        q, t, _, name = images[iid]
        w2c = np.eye(4)
        w2c[:3, :3] = qvec_to_rotmat(q)
        w2c[:3, 3] = t
        poses.append(np.linalg.inv(w2c)[:3, :4])
        names.append(name)
    poses = np.stack(poses, 0) @ np.diag([1., -1., -1., 1.])         # COLMAP (right, down, forward) -> NeRF (right, up, back)
    if load_alphabetical:
        order = np.argsort(names)
        names, poses = [names[i] for i in order], poses[order]
    return names, poses, pixtocam, dist


def pca_align(poses):
    """The first half of camera_utils.transform_poses_pca: rotate the camera centres' principal axes onto x, y, z (largest
    variance first, right-handed) about their mean.  Returns (poses [N, 3, 4], transform [4, 4]) before the y flip and the
    scaling.  The eigenvectors come from np.linalg.eig, as upstream: their signs are LAPACK's and decide the orientation."""
    centres = poses[:, :3, 3]
    mean = centres.mean(0)
    d = centres - mean
    vals, vecs = np.linalg.eig(d.T @ d)
    rot = vecs[:, np.argsort(vals)[::-1]].T
    if np.linalg.det(rot) < 0:
        rot = np.diag([1., 1., -1.]) @ rot
    transform = np.eye(4)
    transform[:3, :3] = rot
    transform[:3, 3] = rot @ -mean
    bottom = np.broadcast_to(np.array([0., 0., 0., 1.]), poses.shape[:-2] + (1, 4))
    return (transform @ np.concatenate([poses, bottom], -2))[..., :3, :4], transform


def transform_poses_pca(poses):
    """camera_utils.transform_poses_pca (camera_utils.py:191-227): pca_align, then a flip about x when the mean camera
    y axis has a negative z component (it points down), and a scale of the centres into [-1, 1]^3.  Returns
    (poses [N, 3, 4], transform [4, 4])."""
    out, transform = pca_align(poses)
    if out.mean(0)[2, 1] < 0:
        out = np.diag([1., -1., -1.]) @ out
        transform = np.diag([1., -1., -1., 1.]) @ transform
    s = 1. / np.max(np.abs(out[:, :3, 3]))
    out[:, :3, 3] *= s
    transform = np.diag([s, s, s, 1.]) @ transform
    return out, transform


def split_indices(n, sample_every, llffhold):
    """(train, test) frame indices (datasets.py:742-761): sample_every >= 1 -> test = 9, 19, ..., train = every
    sample_every-th of the others; otherwise every llffhold-th frame (from 0) is a test frame and the rest train."""
    idx = np.arange(n)
    if sample_every >= 1:
        test = np.arange(9, n, 10)
        rest = sorted(set(range(n)) - set(test.tolist()))
        return np.array(rest[::sample_every], np.int64), test.astype(np.int64)
    return idx[idx % llffhold != 0], idx[idx % llffhold == 0]


def convert_depth(raw, crop_range=0.0):
    """KITTI 16-bit depth PNG values -> metres (datasets.py:640-653): values < 2 are invalid (-256 before the division),
    /256, and with crop_range > 0 depths beyond it are invalid too (-256 after the division, as upstream).  Returns
    float32; every invalid value is negative."""
    d = np.array(raw, np.float32)
    d[d < 2] = -256.
    d /= 256.
    if crop_range > 0:
        d[d > crop_range] = -256.
    return d


def keep_ratio_mask(depths_sup, keep_ratio):
    """depth_keep_ratio (datasets.py:654-661): keep a random keep_ratio share of ALL pixels among the valid ones
    (np.random.seed(0), one uniform per pixel of the stacked frames); the others become invalid (-256)."""
    full = np.count_nonzero(depths_sup > 0) / np.prod(depths_sup.shape)
    if not keep_ratio < full:
        raise ValueError('depth_keep_ratio %g must be below the share of valid supervision pixels (%g)' % (keep_ratio, full))
    np.random.seed(0)
    mask = np.bitwise_and(depths_sup > 0, np.random.uniform(0, 1, depths_sup.shape) < keep_ratio / full)
    out = depths_sup.copy()
    out[~mask] = -256.
    return out


def _listdir(d):
    return sorted(f for f in os.listdir(d) if not f.startswith('.'))


class Scene(object):
    """One COLMAP-format scene as LLFF._load_renderings loads it for configs/360.gin.  Attributes (all frames, COLMAP
    alphabetical order): names, poses [N, 3, 4] (after transform_poses_pca), pixtocam [3, 3] (scaled by the factor),
    distortion, images uint8 [N, H, W, 3], depths_gt / depths_sup float32 [N, H, W] (scene units: metres x scale,
    invalid < 0), scale (= Config.depth_scale), near / far (auto-adjusted), train / test
    indices."""

    def __init__(self, cfg):
        from PIL import Image
        data_dir = cfg['data_dir']
        if not data_dir:
            raise ConfigError('Config.data_dir is not set')
        factor = int(cfg['factor'])
        sfx = '_%d' % factor if factor > 0 else ''
        f = factor if factor > 0 else 1
        self.sparse_dir = os.path.join(data_dir, 'sparse', '0')
        names, poses, pixtocam, dist = load_colmap_poses(self.sparse_dir, cfg['load_alphabetical'])
        self.names = names
        self.pixtocam = (pixtocam @ np.diag([f, f, 1.])).astype(np.float32)
        self.distortion = dist
        colmap_dir, image_dir = os.path.join(data_dir, 'images'), os.path.join(data_dir, 'images' + sfx)
        for d in (image_dir, colmap_dir):
            if not os.path.isdir(d):
                raise ValueError('Image folder %s does not exist.' % d)
        colmap_files = _listdir(colmap_dir)
        to_image = dict(zip(colmap_files, _listdir(image_dir)))
        self.images = np.stack([np.asarray(Image.open(os.path.join(image_dir, to_image[n])).convert('RGB'), np.uint8) for n in names], 0)
        # Depths are always loaded, as upstream does (datasets.py: _load_disps = True): the depth metrics score every run;
        # Config.compute_disp_metrics gates only the depth LOSS (train_utils.py) and the disparity metrics of eval.py.
        gt_dir = os.path.join(data_dir, 'depths_gt' + sfx)
        sup_dir = os.path.join(data_dir, 'depths' + sfx + '_' + cfg['depth_sup_type'])
        # The stages that compute or repair the training split's prior when it goes to the device (device_frames; depth_prior_stages.py):
        # their switches become attributes here, before a folder is read -- a computed prior's folder is not read and need not exist
        stage_attrs, computed, anchor_type, stage_std = PS.scene_switches(cfg)
        self.__dict__.update(stage_attrs)
        for d in (gt_dir,) if computed else (gt_dir, sup_dir):
            if not os.path.isdir(d):
                raise ValueError('Depth folder %s does not exist.' % d)
        to_gt = dict(zip(colmap_files, _listdir(gt_dir)))
        load = lambda d, fn: np.asarray(Image.open(os.path.join(d, fn)), np.float32)
        gt = np.stack([convert_depth(load(gt_dir, to_gt[n])) for n in names], 0)

        def load_prior(d):                                           # a folder of priors in metres: crop range, keep ratio
            if not os.path.isdir(d):
                raise ValueError('Depth folder %s does not exist.' % d)
            to_d = dict(zip(colmap_files, _listdir(d)))
            a = np.stack([convert_depth(load(d, to_d[n]), cfg['depth_crop_range']) for n in names], 0)
            return keep_ratio_mask(a, cfg['depth_keep_ratio']) if cfg['depth_keep_ratio'] > 0 else a
        sup = np.zeros_like(gt) if computed else load_prior(sup_dir)   # (a computed one: the test split's is never touched, no prior)
        self.poses, self.transform = transform_poses_pca(poses)
        self.scale = float(np.sqrt((self.transform[:3, :3] @ self.transform[:3, :3].T)[0, 0]))
        self.near, self.far = float(cfg['near']), float(cfg['far'])
        if cfg['auto_adjust_near_far']:
            self.near, self.far = self.near * self.scale, self.far * self.scale
        self.depths_gt, self.depths_sup = (self.scale * gt).astype(np.float32), (self.scale * sup).astype(np.float32)
        self.__dict__.update(PS.scene_params(self, cfg))             # the stages' parameters, now that the scale is known
        self.depths_anchor = None                                    # the alignment's anchor, loaded the way the prior is, unless a stage computes it
        if anchor_type:
            self.depths_anchor = (self.scale * load_prior(os.path.join(data_dir, 'depths' + sfx + '_' + anchor_type))).astype(np.float32)
        # The standard deviation of the prior, for Config.depth_loss_type = 'gnll' only: the maps of depths{sfx}_{type}_std/ with the
        # prior's conversion and scene scaling (no crop range, no keep ratio), else Config.depth_gnll_std metres at every pixel.
        self.depths_std = self.depth_std_const = None
        self.depth_std_source = None                 # 'folder', 'constant' or the stage's name for it (depth_prior_stages.std_source)
        if DL.needs(cfg.get('depth_loss_type'), 'depth_std') and cfg.get('compute_disp_metrics', True):   # (without the flag: no depth loss)
            std_dir = sup_dir + '_std'
            if os.path.isdir(std_dir):
                to_std = dict(zip(colmap_files, _listdir(std_dir)))
                self.depths_std = (self.scale * np.stack([convert_depth(load(std_dir, to_std[n])) for n in names], 0)).astype(np.float32)
                self.depth_std_source = 'folder'
            elif float(cfg.get('depth_gnll_std', 0.0)) > 0:
                self.depth_std_const = float(np.float32(self.scale * float(cfg['depth_gnll_std'])))
                self.depth_std_source = 'constant'
            else:
                self.depth_std_source = stage_std
            if self.depth_std_source is None:
                raise ValueError('the gnll depth loss needs the standard deviation of the prior: Depth folder %s does not exist and '
                                 'Config.depth_gnll_std = %r (write the maps there, encoded like the prior, or bind a constant in '
                                 'metres)' % (std_dir, cfg.get('depth_gnll_std', 0.0)))
        self.height, self.width = self.images.shape[1:3]
        self.train, self.test = split_indices(len(names), int(cfg['sample_every']), int(cfg['llffhold']))

    def indices(self, split):
        idx = {'train': self.train, 'test': self.test}[split]
        if len(idx) == 0:
            raise ValueError('the %s split of %d frames is empty (sample_every >= 1 takes frames 9, 19, ... as the test split; '
                             'llffhold every llffhold-th frame)' % (split, len(self.names)))
        return idx

    def camera_table(self, split):
        from . import mip360
        return mip360.camera_table(self.pixtocam, self.poses[self.indices(split)], self.distortion)

    def device_frames(self, split, device):
        """A split's frames on the device, once: cams [F, 28], rgb_u8 uint8 [F, H, W, 3], depth_sup / depth_gt float32 [F, H, W] and, in a
        'gnll' run, depth_std float32 [F, H, W] (a constant one is an expanded view of one element).  The train split's prior has been
        through the stages that are on, in the order of depth_prior_stages.STAGES, each of which leaves its rows under
        'depth_<name>_rows' (int64 [F, 4]; the alignment's float64 [F, 8]); the test split is never touched.  What each stage does to
        depth_sup and depth_std: DESIGN.md 8.14."""
        import torch
        idx = self.indices(split)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        out = dict(cams=T(self.camera_table(split)), rgb_u8=T(self.images[idx]), depth_sup=T(self.depths_sup[idx]),
                   depth_gt=T(self.depths_gt[idx]))
        if self.depths_std is not None:
            out['depth_std'] = T(self.depths_std[idx])
        elif self.depth_std_const is not None:
            out['depth_std'] = torch.full((1, 1, 1), self.depth_std_const, device=device).expand(len(idx), self.height, self.width)
        return PS.run_frames(self, idx, device, out) if split == 'train' else out
