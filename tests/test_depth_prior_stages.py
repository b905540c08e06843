"""No GPU: the table of the depth-prior stages (outdoor_nerf_depth_amd/depth_prior_stages.py) -- that it lists the six
stage modules, that both flag surfaces refuse what they refused before the table with the same words (the expected texts below were
copied from ddp_train_nerf.validate_args and mip360_data.Scene.__init__ as they stood before it), the precedence of the sources of a
'gnll' run's standard deviation, and the seam: outside the table and the stage modules no trainer names a stage's switch."""
import itertools
import os
import re
import subprocess
import sys

import pytest

from outdoor_nerf_depth_amd import depth_prior_stages as PS
from outdoor_nerf_depth_amd import mip360_data as D
from tests.test_depth_consistency import write_colmap_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'outdoor_nerf_depth_amd')


def test_the_table_lists_the_six_stage_modules_in_run_order():
    assert [st.name for st in PS.STAGES] == ['mvs', 'points', 'align', 'acc', 'cons', 'comp']
    assert [st.module for st in PS.STAGES] == ['depth_mvs', 'depth_points', 'depth_align', 'depth_accumulate', 'depth_consistency', 'depth_complete']
    bindings = set()
    for f in os.listdir(PKG):                                                    # every module with a load-time *_samplers adapter is a row
        if f.endswith('.py') and re.search(r'^def \w+_samplers\(samplers', open(os.path.join(PKG, f)).read(), re.M):
            bindings.add(f[:-3])
    assert bindings == set(st.module for st in PS.STAGES)
    assert sorted(PS.MIP360_PRINT_ORDER) == sorted(PS.FLAG_ORDER) == sorted(PS.BY_NAME)
    assert [st.source for st in PS.STAGES] == ['mvs', 'points', 'alignment', None, 'consistency', 'completion']
    assert [st.name for st in PS.STAGES if st.computes] == ['mvs', 'points']


def test_the_table_imports_without_torch_ctypes_or_a_binding():
    code = ('import sys; import outdoor_nerf_depth_amd.depth_prior_stages as PS; '
            "bad = [m for m in sys.modules if m.split('.')[0] in ('torch', 'ctypes', 'numpy') or (m.startswith('outdoor_nerf_depth_amd.') and "
            "m != 'outdoor_nerf_depth_amd.depth_prior_stages')]; assert not bad, bad; assert len(PS.STAGES) == 6; print('clean')")
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'clean' in out.stdout, out.stdout[-1000:] + out.stderr[-2000:]


# ------------------------------------------------------------------------------------------------------ the NeRF++ flags
ON = {'cons': ['--depth_cons_views', '2'], 'acc': ['--depth_acc_views', '2'], 'align': ['--depth_align_anchor', 'lidar'],
      'comp': ['--depth_comp_iters', '2'], 'mvs': ['--depth_mvs_views', '2', '--depth_sup_type', 'mvs'],
      'points': ['--depth_points_model', 'm', '--depth_sup_type', 'points']}
FLAG_REFUSALS = [
    (['--depth_cons_views', '17'], '--depth_cons_views = 17: expected 0 (off) .. 16'),
    (['--depth_cons_views', '-1'], '--depth_cons_views = -1: expected 0 (off) .. 16'),
    (ON['cons'], '--depth_cons_views checks the depth prior of a run that trains on it: it needs --use_depth'),
    (['--depth_acc_views', '17'], '--depth_acc_views = 17: expected 0 (off) .. 16'),
    (ON['acc'], '--depth_acc_views densifies the depth prior of a run that trains on it: it needs --use_depth'),
    (ON['align'], '--depth_align_anchor aligns the depth prior of a run that trains on it: it needs --use_depth'),
    (['--use_depth', '--depth_sup_type', 'lidar'] + ON['align'],
     "--depth_align_*: --depth_align_anchor = 'lidar' is the prior itself (depth_sup_type): a prior is aligned to another, metric one"),
    (['--use_depth', '--depth_align_iters', '33'] + ON['align'], '--depth_align_*: iters = 33: expected an integer 0 .. 32'),
    (['--depth_comp_iters', '17'], '--depth_comp_iters = 17: expected 0 (off) .. 16'),
    (ON['comp'], '--depth_comp_iters completes the depth prior of a run that trains on it: it needs --use_depth'),
    (['--use_depth', '--depth_comp_radius', '99'] + ON['comp'], '--depth_comp_*: radius = 99'),
    (['--depth_mvs_views', '17'], '--depth_mvs_views = 17: expected 0 (off) .. 16'),
    (ON['mvs'], '--depth_mvs_views computes the depth prior of a run that trains on it: it needs --use_depth'),
    (['--use_depth', '--depth_mvs_views', '2'],
     '--depth_mvs_views computes the prior that --depth_sup_type gt would read from disk: it needs --depth_sup_type mvs'),
    (['--use_depth', '--depth_mvs_planes', '2'] + ON['mvs'], '--depth_mvs_*: planes = 2'),
    (ON['points'], '--depth_points_model computes the depth prior of a run that trains on it: it needs --use_depth'),
    (['--use_depth', '--depth_points_model', 'm', '--depth_align_anchor', 'lidar'],
     '--depth_points_model computes the prior that --depth_sup_type points or the anchor that --depth_align_anchor points would read from '
     "disk: it needs one of them (they are 'gt' and 'lidar')"),
    (['--use_depth', '--depth_points_occl_radius', '9'] + ON['points'], '--depth_points_*: occl_radius = 9: expected an integer 0 .. 8'),
]


@pytest.mark.parametrize('argv,text', FLAG_REFUSALS, ids=[' '.join(a) for a, _ in FLAG_REFUSALS])
def test_nerfpp_flags_refuse_with_the_words_they_had(argv, text):
    pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    args = T_.config_parser().parse_args(['--expname', 'x', '--synthetic'] + argv)
    with pytest.raises(SystemExit) as e:
        T_.validate_args(args)
    assert str(e.value).startswith(text), str(e.value)


def test_nerfpp_flags_accept_every_stage_and_make_the_std_folder_optional():
    pytest.importorskip('torch')
    from outdoor_nerf_depth_amd import ddp_train_nerf as T_
    parse = lambda argv: T_.config_parser().parse_args(['--expname', 'x', '--synthetic', '--use_depth'] + argv)
    assert PS.check_args(parse([])) == ({'mvs': 0, 'points': '', 'align': '', 'acc': 0, 'cons': 0, 'comp': 0}, dict.fromkeys(PS.BY_NAME))
    for name, argv in ON.items():
        on, target = PS.check_args(parse(argv))
        assert [k for k, v in on.items() if v] == [name] and on[name] == {'align': 'lidar', 'points': 'track'}.get(name, 2)
        assert target[name] == ('prior' if PS.BY_NAME[name].computes else None)
        assert PS.std_source(on, target) == PS.BY_NAME[name].source                                 # (acc: none, the folder stays required)
    # the points as the alignment's anchor: the folder is optional through the alignment
    on, target = PS.check_args(parse(['--depth_points_model', 'm', '--depth_points_vis', 'all', '--depth_sup_type', 'mono', '--depth_align_anchor', 'points']))
    assert on['points'] == 'all' and target['points'] == 'anchor' and PS.std_source(on, target) == 'alignment'
    parsers = [T_.config_parser().format_help()]
    for flag in ('--depth_cons_views', '--depth_acc_views', '--depth_align_anchor', '--depth_comp_iters', '--depth_mvs_views', '--depth_points_model'):
        parsers.append(parsers[-1].split(flag + ' ', 1)[1])                                           # --help lists them in this order
    assert '--depth_gnll_std' in parsers[0].split('--depth_cons_views ')[0] and '--precision' in parsers[-1]


# --------------------------------------------------------------------------------------------------- the MipNeRF-360 Config
@pytest.fixture(scope='module')
def base(tmp_path_factory):
    root = tmp_path_factory.mktemp('stages_colmap')
    write_colmap_scene(str(root), F=10, H=8, W=10)
    return ["Config.data_dir = '%s'" % root]


NOISY, MVS, POINTS = ["Config.depth_sup_type = 'noisy'"], ["Config.depth_sup_type = 'mvs'"], ["Config.depth_sup_type = 'points'"]
OFF = ['Config.compute_disp_metrics = False']
CONFIG_REFUSALS = [
    (NOISY + ['Config.depth_cons_views = 17'], 'Config.depth_cons_views = 17: expected 0 (off) .. 16'),
    (NOISY + ['Config.depth_acc_views = -1'], 'Config.depth_acc_views = -1: expected 0 (off) .. 16'),
    (NOISY + ['Config.depth_comp_iters = 17'], 'Config.depth_comp_iters = 17: expected 0 (off) .. 16'),
    (NOISY + ['Config.depth_mvs_views = 17'], 'Config.depth_mvs_views = 17: expected 0 (off) .. 16'),
    (NOISY + ['Config.depth_mvs_views = 2'],
     "Config.depth_mvs_views = 2 computes the prior that Config.depth_sup_type = 'noisy' would read from disk: it needs Config.depth_sup_type = 'mvs'"),
    (MVS + OFF + ['Config.depth_mvs_views = 2'],
     'Config.depth_mvs_views = 2 computes the depth prior of a run that trains on it: it needs Config.compute_disp_metrics = True'),
    (MVS + ['Config.depth_mvs_views = 2', 'Config.depth_mvs_planes = 2'], 'Config.depth_mvs_*: planes = 2'),
    (NOISY + ["Config.depth_points_vis = 'track'", "Config.depth_align_anchor = 'gt'"],
     "Config.depth_points_vis = 'track' computes the prior that Config.depth_sup_type = 'points' or the anchor that Config.depth_align_anchor = "
     "'points' would read from disk: it needs one of them (they are 'noisy' and 'gt')"),
    (POINTS + OFF + ["Config.depth_points_vis = 'all'"],
     "Config.depth_points_vis = 'all' computes the depth prior of a run that trains on it: it needs Config.compute_disp_metrics = True"),
    (POINTS + ["Config.depth_points_vis = 'most'"], "Config.depth_points_vis = 'most': expected '' (off), 'track' or 'all'"),
    (POINTS + ["Config.depth_points_vis = 'track'", 'Config.depth_points_occl_radius = 9'],
     'Config.depth_points_*: occl_radius = 9: expected an integer 0 .. 8'),
    (NOISY + ["Config.depth_align_anchor = 'noisy'"],
     "Config.depth_align_anchor = 'noisy' is the prior itself (depth_sup_type): a prior is aligned to another, metric one"),
    (NOISY + ["Config.depth_align_anchor = 'gt'", 'Config.depth_align_iters = 40'], 'iters = 40: expected an integer 0 .. 32'),
    (NOISY + ['Config.depth_comp_iters = 2', 'Config.depth_comp_radius = 99'], 'Config.depth_comp_*: radius = 99'),
]


@pytest.mark.parametrize('bindings,text', CONFIG_REFUSALS, ids=['; '.join(b[1:]) for b, _ in CONFIG_REFUSALS])
def test_mip360_config_refuses_with_the_words_it_had(base, bindings, text):
    with pytest.raises(D.ConfigError) as e:
        D.Scene(D.parse_gin(bindings=base + bindings))
    assert str(e.value).startswith(text), str(e.value)


def test_mip360_config_keeps_the_attributes_and_accepts_the_repairs_without_the_depth_loss(base):
    s = D.Scene(D.parse_gin(bindings=base + NOISY))
    assert (s.depth_mvs_views, s.depth_points_vis, s.depth_points_target, s.depth_align_anchor, s.depths_anchor, s.depth_acc_views,
            s.depth_cons_views, s.depth_comp_iters, s.depth_std_source) == (0, '', None, '', None, 0, 0, 0, None)
    assert set(s.depth_cons_cfg) == set(k for k in D.CONFIG_DEFAULTS if k.startswith('depth_cons_')) and s.depth_acc_cfg['depth_acc_occl_radius'] == 2
    assert not [k for k in vars(s) if k.endswith('_prm')]
    # only a stage that computes the prior refuses a run without the depth loss
    s = D.Scene(D.parse_gin(bindings=base + NOISY + OFF + ['Config.depth_cons_views = 2', 'Config.depth_acc_views = 3', "Config.depth_align_anchor = 'gt'",
                                                           'Config.depth_comp_iters = 4']))
    assert (s.depth_cons_views, s.depth_acc_views, s.depth_align_anchor, s.depth_comp_iters) == (2, 3, 'gt', 4) and s.depths_anchor is not None
    assert s.depth_align_prm['iters'] == 10 and s.depth_comp_prm['iters'] == 4 and s.depth_acc_cfg['depth_acc_views'] == 3


# the switches that can be bound together, by the source they stand for; depth_sup_type decides which of mvs and points can be on
SWITCH = {'points': POINTS + ["Config.depth_points_vis = 'track'"], 'mvs': MVS + ['Config.depth_mvs_views = 2'],
          'alignment': ["Config.depth_align_anchor = 'gt'"], 'consistency': ['Config.depth_cons_views = 2'], 'completion': ['Config.depth_comp_iters = 2']}
PRECEDENCE = ('folder', 'constant', 'points', 'mvs', 'alignment', 'consistency', 'completion')


def test_std_source_follows_the_precedence_over_every_pair(base):
    from PIL import Image
    import numpy as np
    root = base[0].split("'")[1]
    gnll = ["Config.depth_loss_type = 'gnll'"]
    pairs = [p for p in itertools.combinations(PRECEDENCE, 2) if set(p) != {'points', 'mvs'}]       # (each needs its own depth_sup_type)
    assert len(pairs) == 20
    for first, second in pairs:
        sup = 'points' if 'points' in (first, second) else 'mvs' if 'mvs' in (first, second) else 'noisy'
        bindings = ["Config.depth_sup_type = '%s'" % sup]
        std_dir = os.path.join(root, 'depths_%s_std' % sup)
        for name in (first, second):
            if name == 'folder':
                os.makedirs(std_dir)
                for f in os.listdir(os.path.join(root, 'depths_gt')):
                    Image.fromarray(np.full((8, 10), 64, np.uint16)).save(os.path.join(std_dir, f))
            elif name == 'constant':
                bindings.append('Config.depth_gnll_std = 0.1')
            else:
                bindings += [b for b in SWITCH[name] if 'depth_sup_type' not in b]
        try:
            s = D.Scene(D.parse_gin(bindings=base + bindings + gnll))
        finally:
            if os.path.isdir(std_dir):
                for f in os.listdir(std_dir):
                    os.remove(os.path.join(std_dir, f))
                os.rmdir(std_dir)
        assert s.depth_std_source == first, (first, second, s.depth_std_source)
    for name in PRECEDENCE[2:]:                                                                     # and each one alone
        assert D.Scene(D.parse_gin(bindings=base + NOISY + SWITCH[name] + gnll)).depth_std_source == name
    with pytest.raises(ValueError, match='the gnll depth loss needs the standard deviation of the prior'):
        D.Scene(D.parse_gin(bindings=base + NOISY + ['Config.depth_acc_views = 2'] + gnll))          # the accumulation names no source
    anchored = D.Scene(D.parse_gin(bindings=base + NOISY + ["Config.depth_align_anchor = 'points'", "Config.depth_points_vis = 'track'"] + gnll))
    assert anchored.depth_std_source == 'alignment' and anchored.depth_points_target == 'anchor'    # the points as the anchor give none


# ---------------------------------------------------------------------------------------------------------------- the seam
def test_no_trainer_names_a_stage_switch():
    """outside depth_prior_stages.py and the stage modules, the trainers and the scene reader name no depth_<stage>_ key: what they
    need of a stage they ask of the table.  The exception is Config's dictionary of defaults."""
    found = []
    for f in ('ddp_train_nerf.py', 'mip360_train.py', 'mip360_data.py'):
        text = open(os.path.join(PKG, f)).read()
        if f == 'mip360_data.py':
            head, rest = text.split('CONFIG_DEFAULTS = dict(', 1)
            defaults, tail = rest.split('\n\n', 1)
            assert len(re.findall(r'depth_(cons|acc|align|comp|mvs|points)_\w+=', defaults)) > 40
            text = head + '\n' * defaults.count('\n') + '\n\n' + tail
        found += ['%s:%d: %s' % (f, i + 1, line.strip()[:80]) for i, line in enumerate(text.split('\n'))
                  if re.search(r'depth_(cons|acc|align|comp|mvs|points)_', line)]
    assert not found, found
