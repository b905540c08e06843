"""CPU (no GPU, no library): the table of depth losses (outdoor_nerf_depth_amd/depth_losses.py) against everything
that used to spell the names out by itself -- the libraries' code tables, the NeRF++ CLI's choices, what NerfppTrainer accepts and
refuses -- and the condition that keeps it the only place that knows the names: no other module of the package compares a depth
loss type against 'ssi' / 'gnll'."""
import ast
import glob
import os
import subprocess
import sys

import pytest

from outdoor_nerf_depth_amd import depth_losses as DL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'outdoor_nerf_depth_amd')
NOT_A_DEPTH_LOSS = 'rgbonly'              # the NeRF++ head's code 0: NerfppTrainer(use_depth=False), no choice of --depth_loss_type


def test_names_per_path():
    from outdoor_nerf_depth_amd import _lib, mip360
    from outdoor_nerf_depth_amd import ddp_train_nerf as T
    choices = next(a for a in T.config_parser()._actions if a.dest == 'depth_loss_type').choices
    assert choices == ['mse', 'kl', 'los', 'l1', 'nll', 'ssi', 'gnll']               # today's list, the dead names included
    assert set(choices) - set(DL.DEAD) == set(DL.names('nerfpp')) - {NOT_A_DEPTH_LOSS} and set(DL.DEAD) == {'los', 'nll'}
    assert DL.names('nerfpp') == tuple(_lib.LOSS_TYPES) + DL.names('nerfpp', DL.AFTER) == ('rgbonly', 'mse', 'l1', 'kl', 'ssi', 'gnll')
    assert DL.names('mip360') == mip360.DEPTH_LOSS_TYPES == tuple(mip360.DEPTH_TYPES) + (mip360.SSI, mip360.GNLL)
    assert DL.names('mip360', DL.AFTER) == ('kl_ray', 'urf_ray', 'ssi', 'gnll')
    assert (mip360.SSI, mip360.GNLL) == ('ssi', 'gnll')


def test_core_codes_are_the_libraries():
    from outdoor_nerf_depth_amd import _lib, mip360
    seen = {'nerfpp': 0, 'mip360': 0}
    for name, row in DL.LOSSES.items():
        for path, codes in (('nerfpp', _lib.LOSS_TYPES), ('mip360', mip360.DEPTH_TYPES)):
            kind = getattr(row, path)
            assert kind is None or kind == DL.AFTER or type(kind) is int, (name, path)
            if type(kind) is int:
                assert codes[name] == kind, (name, path)
                seen[path] += 1
            elif kind is None:
                assert name not in codes, (name, path)
        # an after-call brings its adapter; only a loss that runs outside the heads has anything to refuse, to log or to be given
        is_after = DL.AFTER in (row.nerfpp, row.mip360)
        assert (row.call is not None) == is_after and (is_after or not (row.inputs or row.refuses or row.log or row.stats or row.extra))
        assert set(row.inputs) <= set(DL.INPUTS) and set(row.refuses) <= set(DL.REFUSAL) and set(row.reads) <= {'weights', 'x', 'pred'}
    # kl_ray / urf_ray keep their codes in DEPTH_TYPES (depth_loss_rays passes them on) although they run as after-calls
    assert seen == {'nerfpp': len(_lib.LOSS_TYPES), 'mip360': len(mip360.DEPTH_TYPES) - 2} and len(mip360.DEPTH_TYPES) == 8


def _trainer(name, **kw):
    from outdoor_nerf_depth_amd.trainer import NerfppTrainer
    # no levels, no side streams: the whole constructor runs on a host without a device
    return NerfppTrainer('cpu', use_depth=True, depth_loss_type=name, level_params=[], cascade_samples=(), overlap_allreduce=False, **kw)


@pytest.mark.parametrize('name', [n for n in DL.LOSSES if n is not None] + ['nll', 'los', 'huber'])
def test_nerfpp_trainer_accepts_what_the_table_says(name):
    pytest.importorskip('torch')
    row = DL.LOSSES.get(name)
    if row is not None and row.nerfpp is not None:
        assert _trainer(name).loss_type == name
    else:
        with pytest.raises(ValueError, match='dead code there'):
            _trainer(name)


def test_refused_examples_are_refused():
    assert all(n not in DL.names('nerfpp') for n in ('urf', 'kl_ray', 'nll'))


@pytest.mark.parametrize('name', DL.names('nerfpp'))
def test_nerfpp_trainer_refuses_the_options_the_table_says(name):
    pytest.importorskip('torch')
    reasons = {'fuse_loss': 'the fused compositing backward forms the depth gradient itself, from mse / l1 / kl only',
               'optim_autoexpo': "the auto-exposure gradient is taken from the loss head's own depth term"}
    assert DL.REFUSAL == reasons
    for option, kw in (('fuse_loss', dict(fuse_loss=True)), ('optim_autoexpo', dict(optim_autoexpo=True, img_names=['a']))):
        if option in DL.LOSSES[name].refuses:
            with pytest.raises(ValueError) as e:
                _trainer(name, **kw)
            assert "depth_loss_type '%s' and %s cannot be combined: %s" % (name, option, reasons[option]) == str(e.value)
        else:
            t = _trainer(name, **kw)
            assert t.fuse_loss == (option == 'fuse_loss') and (t.autoexpo is not None) == (option == 'optim_autoexpo')
    assert set(DL.LOSSES[name].refuses) == ({'fuse_loss', 'optim_autoexpo'} if name in ('ssi', 'gnll') else set())


def test_inputs_and_log_tails():
    import numpy as np
    assert [n for n in DL.LOSSES if DL.needs(n, 'depth_std')] == ['gnll'] and [n for n in DL.LOSSES if DL.needs(n, 'cam_idx')] == ['ssi']
    assert not DL.needs('huber', 'depth_std') and not DL.needs(None, 'cam_idx')
    assert {n: r.log[0] for n, r in DL.LOSSES.items() if r.log} == {'ssi': 'ssi_fit', 'gnll': 'gnll_gated'}

    class Stats(object):                   # what depth_log_tail asks of a device tensor
        def __init__(self, a):
            self.a = np.asarray(a, np.float32)

        def __getitem__(self, k):
            return Stats(self.a[k])

        def reshape(self, *shape):
            return Stats(self.a.reshape(*shape))

        def cpu(self):
            return self

        def numpy(self):
            return self.a
    assert DL.depth_log_tail('ssi', Stats([[9, 9], [8, 2]])) == ' ssi_fit=0.250'                     # MipNeRF-360: [levels, 2]
    assert DL.depth_log_tail('gnll', Stats([[9, 9, 9], [3, 1, 0]])) == ' gnll_gated=0.333'           # MipNeRF-360: [levels, 3]
    assert DL.depth_log_tail('gnll', [Stats([[9, 9, 9]]), Stats([[0, 0, 0]])]) == ' gnll_gated=0.000'  # NeRF++: [levels][1, 3]
    assert DL.depth_log_tail('gnll', None) == DL.depth_log_tail('mse', Stats([[1, 1]])) == DL.depth_log_tail('huber', None) == ''

    class Trainer(object):
        last_gnll_stats = 'kept'
    # the NeRF++ trainer keeps no ssi stats, so its log lines get no ssi_fit
    assert DL.kept_stats(Trainer(), 'gnll') == 'kept' and DL.kept_stats(Trainer(), 'ssi') is None and DL.kept_stats(Trainer(), 'mse') is None


def _compares_a_name(node):
    """Is `node` a comparison one of whose sides is the literal 'ssi' / 'gnll' (alone or in a tuple / list / set) or the name SSI /
    GNLL (bare or as an attribute)?"""
    def names_one(e):
        if isinstance(e, ast.Constant):
            return e.value in ('ssi', 'gnll')
        if isinstance(e, ast.Name):
            return e.id in ('SSI', 'GNLL')
        if isinstance(e, ast.Attribute):
            return e.attr in ('SSI', 'GNLL')
        if isinstance(e, (ast.Tuple, ast.List, ast.Set)):
            return any(names_one(x) for x in e.elts)
        return False
    return isinstance(node, ast.Compare) and any(names_one(e) for e in [node.left] + list(node.comparators))


def test_the_checker_sees_what_it_is_for():
    for text in ("t == 'ssi'", "'gnll' != t", "t in ('ssi', 'gnll')", 'tr.depth_loss_type == M.SSI', 'GNLL == t', "t not in ['gnll']"):
        assert any(_compares_a_name(n) for n in ast.walk(ast.parse(text))), text
    for text in ("x = {SSI: 1}.get(t)", "assert T == tuple(D) + (SSI, GNLL)", "f('ssi')", "'ssi_fit=%d' % n == s", "SSI = 'ssi'"):
        assert not any(_compares_a_name(n) for n in ast.walk(ast.parse(text))), text


def test_no_module_compares_a_depth_loss_type_against_a_name():
    """the seam: outside the table and the two bindings themselves, nothing asks `== 'ssi'` / `== 'gnll'` / `== SSI` / `== GNLL`"""
    own = ('depth_losses.py', 'depth_ssi.py', 'depth_gnll.py')
    files = [p for p in sorted(glob.glob(os.path.join(PKG, '*.py'))) if os.path.basename(p) not in own]
    assert len(files) > 20
    found = []
    for path in files:
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if _compares_a_name(node):
                found.append('%s:%d' % (os.path.basename(path), node.lineno))
    assert not found, found


def test_the_table_imports_without_torch_or_a_binding():
    code = ('import sys; import outdoor_nerf_depth_amd.depth_losses as DL; '
            "bad = [m for m in sys.modules if m == 'torch' or m.startswith('torch.') or (m.startswith('outdoor_nerf_depth_amd.') and "
            "m != 'outdoor_nerf_depth_amd.depth_losses')]; assert not bad, bad; assert DL.needs('gnll', 'depth_std'); print('clean')")
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'clean' in out.stdout, out.stdout[-1000:] + out.stderr[-2000:]
