"""CPU (no GPU): per-image appearance embeddings (GLO) of the MipNeRF-360 path -- the gin bindings, the frames / embeddings
check, the header's declarations and the argument checks of the two entry points."""
import os
import re

import numpy as np
import pytest

from outdoor_nerf_depth_amd import mip360_data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_gin_accepts_the_glo_bindings(tmp_path):
    cfg = D.parse_gin(bindings=['Model.num_glo_features = 4'])
    assert cfg['num_glo_features'] == 4 and cfg['num_glo_embeddings'] == 1000
    assert D.parse_gin()['num_glo_features'] == 0
    cfg = D.parse_gin(bindings=['Model.num_glo_features = 2', 'Model.num_glo_embeddings = 64'])
    assert (cfg['num_glo_features'], cfg['num_glo_embeddings']) == (2, 64)
    # the bindings of the reference's 360_glo4.gin that differ from 360.gin's, next to two it shares, written by hand
    gin = tmp_path / '360_glo4.gin'
    gin.write_text("Config.factor = 4\nModel.raydist_fn = @jnp.reciprocal\nModel.num_glo_features = 4\nModel.opaque_background = True\n"
                   'NerfMLP.net_width = 1024\n')
    cfg = D.parse_gin([str(gin)])
    assert cfg['num_glo_features'] == 4 and cfg['factor'] == 4


@pytest.mark.parametrize('binding', ['Model.num_glo_features = 5', 'Model.num_glo_features = -1', 'Model.num_glo_features = 4.0',
                                     'Model.num_glo_features = True', 'Model.num_glo_embeddings = 0', 'NerfMLP.net_width = 512',
                                     'Model.num_levels = 4'])
def test_parse_gin_rejects_what_the_kernels_do_not_implement(binding):
    with pytest.raises(D.ConfigError, match=re.escape(binding.split(' = ')[0])):
        D.parse_gin(bindings=[binding])


def test_five_features_says_why():
    with pytest.raises(D.ConfigError, match='column 287 stays'):
        D.parse_gin(bindings=['Model.num_glo_features = 5'])


def test_more_frames_than_embeddings_raises_before_the_library_is_loaded(monkeypatch):
    from outdoor_nerf_depth_amd import mip360 as M
    from outdoor_nerf_depth_amd import mip360_train as T

    def no_lib():
        raise AssertionError('the library was loaded before the configuration was checked')
    monkeypatch.setattr(M, 'lib', no_lib)
    cfg = D.parse_gin(bindings=['Model.num_glo_features = 4', 'Model.num_glo_embeddings = 10'])
    with pytest.raises(D.ConfigError, match=r'Number of training images \(11\) exceeds Model.num_glo_embeddings = 10'):
        T.make_trainer(cfg, 'cpu', n_train_frames=11)
    with pytest.raises(D.ConfigError):
        D.check_glo_frames(cfg, 11)
    D.check_glo_frames(cfg, 10)
    D.check_glo_frames(D.parse_gin(bindings=['Model.num_glo_embeddings = 10']), 500)          # without features nothing to check


def test_trainer_shape_checks_need_no_gpu():
    from outdoor_nerf_depth_amd import mip360 as M
    assert M.mlp_shapes(M.NERF_CFG)[10] == (283, 128) and M.mlp_shapes(M.NERF_CFG, 4)[10] == (287, 128)
    assert M.mlp_shapes(M.PROP_CFG, 4) == M.mlp_shapes(M.PROP_CFG)
    for bad in (5, -1, 2.0):
        with pytest.raises(M.Mip360Error, match='num_glo_features'):
            M.check_glo_shape(bad, 1000)
    e = M.init_glo_embed(1000, 4, np.random.RandomState(3))
    assert e.shape == (1000, 4) and e.dtype == np.float32 and abs(e.std() - 0.5) < 0.02          # normal, std 1 / sqrt(G)


def test_header_declares_the_entry_points_and_keeps_abi_9():
    text = open(os.path.join(ROOT, 'include', 'mip360_hip.h')).read()
    assert re.search(r'#define MIP360_ABI_VERSION 9\b', text)
    for name in ('mip360_dir_glo_encode', 'mip360_glo_backward', 'mip360_glo_revision'):
        assert re.search(r'\bint %s\(' % name, text), name


def test_entry_points_validate_arguments_without_a_gpu():
    from outdoor_nerf_depth_amd import mip360 as M
    lib = M.lib()
    assert lib.mip360_abi_version() == M.ABI_VERSION == 9 and lib.mip360_glo_revision() == M.GLO_REVISION == 1
    d = 64                                                     # a non-null, 16-byte aligned value no failing call dereferences
    err = lambda: lib.mip360_last_error()
    # mip360_dir_glo_encode(stream, n_rays, n_samples, viewdirs, embed, E, G, cam_idx, cam_stride, out, ld, col0, width)
    assert lib.mip360_dir_glo_encode(None, 16, 1, None, d, 8, 4, d, 1, None, 32, 0, 32) == 1 and b'non-null' in err()
    assert lib.mip360_dir_glo_encode(None, 0, 1, d, d, 8, 4, d, 1, d, 32, 0, 32) == 1
    assert lib.mip360_dir_glo_encode(None, 16, 1, d, d, 8, 5, d, 1, d, 32, 0, 32) == 1 and b'n_features <= 4' in err()
    assert lib.mip360_dir_glo_encode(None, 16, 1, d, d, 8, -1, d, 1, d, 32, 0, 32) == 1
    assert lib.mip360_dir_glo_encode(None, 16, 1, d, None, 8, 4, d, 1, d, 32, 0, 32) == 1 and b'cam_idx needs embed' in err()
    assert lib.mip360_dir_glo_encode(None, 16, 1, d, d, 0, 4, d, 1, d, 32, 0, 32) == 1
    assert lib.mip360_dir_glo_encode(None, 16, 1, d, d, 8, 4, d, 0, d, 32, 0, 32) == 1
    assert lib.mip360_dir_glo_encode(None, 16, 1, d, d, 8, 4, d, 1, d, 32, 0, 30) == 1 and b'27 + n_features <= width' in err()
    assert lib.mip360_dir_glo_encode(None, 16, 1, d, d, 8, 4, d, 1, d, 32, 8, 32) == 1
    # mip360_glo_backward(stream, n_rays, S, G, E, d_hz, ld_dhz, wb_view, ld_wb, cam_idx, cam_stride, partial, g_embed)
    ok = [None, 16, 32, 4, 8, d, 128, d, 128, d, 1, d, d]
    def call(**kw):
        names = ['stream', 'n_rays', 'S', 'G', 'E', 'd_hz', 'ld_dhz', 'wb', 'ld_wb', 'cam', 'stride', 'partial', 'g_embed']
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.mip360_glo_backward(*a)
    for ptr in ('d_hz', 'wb', 'cam', 'partial', 'g_embed'):
        assert call(**{ptr: None}) == 1 and b'non-null' in err(), ptr
    assert call(G=5) == 1 and b'n_features <= 4' in err()
    assert call(G=0) == 1
    assert call(ld_dhz=64) == 1 and b'ld_dhz' in err()
    assert call(ld_dhz=132) == 1
    assert call(ld_wb=96) == 1
    assert call(n_rays=0) == 1 and b'n_rays > 0' in err()
    assert call(n_rays=-4) == 1
    assert call(S=0) == 1
    assert call(E=0) == 1
    assert call(stride=0) == 1
    assert call(d_hz=72) == 1 and b'aligned' in err()
