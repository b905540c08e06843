"""Per-image appearance embeddings (GLO) of the MipNeRF-360 path on the GPU: mip360_dir_glo_encode / mip360_glo_backward through
the C ABI, the fused view branch on a table that carries embeddings, the trainer with Model.num_glo_features = 4 and 0,
checkpoints and the CLIs.  The float64 reference is tests/mip360_glo_reference.py.

Measured on an MI355X (profiles/r10_mip360_glo_error.json, profiles/r10_mip360_glo_train.json):
* embedding gradient against float64 on the identical bf16 operands, max |err| / sum |products| over the case list: 1.2e-8
  (GRAD_ERR_MEASURED); the gate is 4x that (the cap of 1e-5 is far away);
* the training run with per-frame colour gains, data loss averaged over the last 50 of 400 steps: 0.0741 with G = 4 against
  0.0910 with G = 0, a gap of 0.0168 = 63 standard errors of those means (TRAIN_GAP_MEASURED); the gate is half the gap.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import mip360_glo_reference as R
from tests.test_gpu_mip360_fm import M, N, T, bf, dev, round_bf16   # noqa: F401  (fixtures / helpers)

pytestmark = pytest.mark.gpu

GRAD_ERR_MEASURED = 1.1994554704626308e-08       # profiles/r10_mip360_glo_error.json: the worst case (every ray its own camera)
GRAD_ERR_GATE = min(4 * GRAD_ERR_MEASURED, 1e-5)
TRAIN_GAP_MEASURED = 0.016844858825206754        # profiles/r10_mip360_glo_train.json: 0.09096 (G = 0) - 0.07412 (G = 4), 63 standard errors
TRAIN_GAP_GATE = 0.5 * TRAIN_GAP_MEASURED


def I32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev())


def bits(t):
    return N(t.view(torch.int16))


def _viewdirs(rs, n):
    vd = rs.randn(n, 3).astype(np.float32)
    return vd / np.linalg.norm(vd, axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------------------ table
@pytest.mark.parametrize('n_rays,G,E', [(64, 4, 12), (256, 1, 1000), (4096, 4, 1000), (100, 3, 7)])
def test_table_is_dir_encode_plus_the_gathered_embedding(M, n_rays, G, E):
    rs = np.random.RandomState(n_rays + G)
    vd, embed = T(_viewdirs(rs, n_rays)), T(rs.randn(E, G).astype(np.float32))
    cam = rs.randint(0, E, n_rays)
    L = M.lib()
    want = torch.full((n_rays, 32), 7.0, dtype=torch.bfloat16, device=dev())
    M._check(L.mip360_dir_encode(M._stream(), n_rays, 1, M._p(vd), M._p(want), 32, 0, 32), 'dir_encode')

    def table(cam_t, stride, g=G, emb=embed):
        out = torch.full((n_rays, 32), 7.0, dtype=torch.bfloat16, device=dev())
        M._check(L.mip360_dir_glo_encode(M._stream(), n_rays, 1, M._p(vd), M._p(emb), E, g, M._p(cam_t), stride, M._p(out), 32, 0, 32),
                 'dir_glo_encode')
        return out
    np.testing.assert_array_equal(bits(table(None, 1)), bits(want))                  # zero_glo: dir_encode's bytes
    np.testing.assert_array_equal(bits(table(I32(cam), 1, g=0, emb=None)), bits(want))   # G = 0: likewise
    gathered = bits(embed.to(torch.bfloat16)[torch.from_numpy(cam).to(dev())])
    pix = np.stack([cam, rs.randint(0, 40, n_rays), rs.randint(0, 32, n_rays)], -1)
    for cam_t, stride in ((I32(cam), 1), (I32(pix), 3)):
        got = bits(table(cam_t, stride))
        np.testing.assert_array_equal(got[:, :27], bits(want)[:, :27])
        np.testing.assert_array_equal(got[:, 27:27 + G], gathered)
        assert (got[:, 27 + G:] == 0).all()
    # the broadcast form (the row-major fallback writes the view layer's input directly): every sample row = its ray's table row
    S = 4
    out = torch.full((n_rays * S, 288), 7.0, dtype=torch.bfloat16, device=dev())
    M.dir_glo_encode(vd, n_rays, S, out, 288, 256, 32, (embed, I32(cam)))
    np.testing.assert_array_equal(bits(out[:, 256:].contiguous()), np.repeat(bits(table(I32(cam), 1)), S, 0))
    assert (N(out[:, :256]) == 7.0).all()
    with pytest.raises(M.Mip360Error, match='outside the %d embedding rows' % E):
        M.dir_glo_encode(vd, n_rays, 1, out, 32, 0, 32, (embed, np.full(n_rays, E, np.int32)))


# ---------------------------------------------------------------------------------------------------------- forward
def _forward_problem(rs, n_rays, S, G, E):
    rows = n_rays * S
    bott = round_bf16(rs.randn(rows, 256).astype(np.float32))
    vd = _viewdirs(rs, n_rays)
    w1 = round_bf16((rs.randn(128, 288) * np.sqrt(2.0 / (283 + G))).astype(np.float32))
    w1[:, 283 + G:] = 0                                        # (the packing never writes the padding columns)
    w2 = round_bf16((rs.randn(3, 128) / np.sqrt(128)).astype(np.float32))
    b1, b2 = (rs.randn(128) * 0.1).astype(np.float32), (rs.randn(3) * 0.1).astype(np.float32)
    embed = (rs.randn(E, G) * 0.5).astype(np.float32)
    cam = rs.randint(0, E, n_rays)
    return dict(rows=rows, bott=bott, vd=vd, w1=w1, w2=w2, b1=b1, b2=b2, embed=embed, cam=cam)


@pytest.mark.parametrize('n_rays,G', [(64, 4), (64, 1), (4096, 4)])
def test_view_branch_fm_reads_the_embedding_columns(M, n_rays, G):
    """mip360_view_branch_fm on a table with embeddings and non-zero weight rows 283..283+G-1: (a) against the launches it replaces,
    by the method and gates of test_gpu_mip360_prop.py::test_view_branch_fm_equals_the_launches_it_replaces; (b) against the
    float64 reference on the same bf16-rounded operands at that test's gates for a bf16 dense layer (rtol 2^-7, atol 2e-3 for the
    hidden layer; 2e-6 for the colours given the kernel's own hidden layer).

    The colours of (a): that test's flat 2e-4 holds where the two hidden layers agree bit for bit.  Where they differ by the bf16
    ulp the hidden-layer gate allows (summation order), the difference reaches the colours through the second layer and the
    sigmoid, whose slope is at most (1 + 2 rgb_padding) / 4: |d rgb| <= 0.2505 sum_j |d h_j| |w2_j|.  With 64 rays and that test's
    scale of operands no such element exceeds 2e-4 (the flat gate is kept for the 64-ray, G = 4 case); among the 16.8 million
    hidden values of the training shape some do, so the gate is 2e-4 plus that propagated bound, row by row."""
    S, E = 32, 12
    P = _forward_problem(np.random.RandomState(21 + G), n_rays, S, G, E)
    rows, w1, w2, b1, b2 = P['rows'], P['w1'], P['w2'], P['b1'], P['b2']
    bott_fm, w1_fm = M.to_fm(bf(P['bott'])), M.to_fm(bf(w1))
    w2p = np.zeros((32, 128), np.float32)
    w2p[:3] = w2
    w2_fm = M.to_fm(bf(w2p))

    class PK(object):
        w_fm = {2: w1_fm, 3: w2_fm}
        b = {2: T(b1), 3: T(b2)}
    embed_t, cam_t, vd_t = T(P['embed']), I32(P['cam']), T(P['vd'])
    view_in = torch.full((rows, 288), 9.0, dtype=torch.bfloat16, device=dev())
    h = torch.full((rows, 128), 9.0, dtype=torch.bfloat16, device=dev())
    rgb = torch.empty(rows, 3, device=dev())
    M.view_branch_fm(PK, 0, bott_fm, rows, S, vd_t, view_in, h, rgb, glo=(embed_t, cam_t))
    # (a) the launches it replaces; the embedding columns are copied in by the host
    want_in = torch.empty(rows, 288, dtype=torch.bfloat16, device=dev())
    M.from_fm(bott_fm, rows, 256, out=want_in)
    M._check(M.lib().mip360_dir_encode(M._stream(), n_rays, S, M._p(vd_t), M._p(want_in), 288, 256, 32), 'dir_encode')
    cam_rows = torch.from_numpy(np.repeat(P['cam'], S)).to(dev())
    want_in[:, 283:283 + G] = embed_t.to(torch.bfloat16)[cam_rows]
    want_h = torch.empty(rows, 128, dtype=torch.bfloat16, device=dev())
    M.linear(want_in, bf(w1), T(b1), act=1, out_bf16=want_h, m=rows, n=128, k=288)
    want_rgb = torch.empty(rows, 3, device=dev())
    M.linear(want_h, bf(w2), T(b2), act=3, act_param=M.RGB_PADDING, out_f32=want_rgb, m=rows, n=3, k=128)
    np.testing.assert_array_equal(N(view_in), N(want_in))
    gh, wh = N(h), N(want_h)
    assert (gh != wh).mean() < 2e-3
    np.testing.assert_allclose(gh, wh, rtol=2 ** -7, atol=1e-6)
    allowed = 2e-4 + 0.2505 * np.abs(gh.astype(np.float64) - wh.astype(np.float64)) @ np.abs(w2.astype(np.float64)).T
    d_rgb = np.abs(N(rgb).astype(np.float64) - N(want_rgb).astype(np.float64))
    print('view branch (%d rays, G = %d): max |rgb - replaced launches| = %.3e, rows over 2e-4: %d' % (n_rays, G, d_rgb.max(), (d_rgb > 2e-4).any(-1).sum()))
    assert (d_rgb <= allowed).all(), float((d_rgb - allowed).max())
    if (n_rays, G) == (64, 4):
        np.testing.assert_allclose(N(rgb), N(want_rgb), rtol=0, atol=2e-4)
    # (b) float64 on the bf16-rounded operands: the reference gathers the embedding itself
    emb64 = torch.from_numpy(round_bf16(P['embed']).astype(np.float64))
    dirs = round_bf16(R.dir_features(P['vd']).numpy().astype(np.float32))
    x = R.view_input(P['bott'], np.repeat(dirs, S, 0), emb64, np.repeat(P['cam'], S))
    assert x.shape[1] == 283 + G
    ref_rgb, ref_h = R.view_branch(x, w1[:, :283 + G].T, b1, w2.T, b2)
    np.testing.assert_allclose(gh, ref_h.numpy(), rtol=2 ** -7, atol=2e-3)
    raw = gh.astype(np.float64) @ w2.astype(np.float64).T + b2
    np.testing.assert_allclose(N(rgb), 1 / (1 + np.exp(-raw)) * (1 + 2 * M.RGB_PADDING) - M.RGB_PADDING, rtol=0, atol=2e-6)
    np.testing.assert_allclose(N(rgb), ref_rgb.numpy(), rtol=0, atol=1.5e-2)          # (test_gpu_mip360.py: rgb against the bf16 reference)
    # the embedding is live: without it (zero vector) the reference moves by more than the gate above, and so does the kernel
    zero_rgb, zero_h = R.view_branch(R.view_input(P['bott'], np.repeat(dirs, S, 0), torch.zeros_like(emb64), np.repeat(P['cam'], S)),
                                     w1[:, :283 + G].T, b1, w2.T, b2)
    assert np.abs(zero_h.numpy() - ref_h.numpy()).max() > 10 * 2e-3
    rgb0 = torch.empty(rows, 3, device=dev())
    M.view_branch_fm(PK, 0, bott_fm, rows, S, vd_t, None, None, rgb0)
    assert np.abs(N(rgb0) - N(rgb)).max() > 1e-3
    np.testing.assert_allclose(N(rgb0), zero_rgb.numpy(), rtol=0, atol=1.5e-2)


# ------------------------------------------------------------------------------------------------ embedding gradient
GRAD_CASES = [  # (name, n_rays, S, G, E, camera assignment)
    ('one_camera', 256, 32, 4, 12, lambda rs, n, E: np.full(n, 5)),
    ('own_camera', 256, 32, 4, 256, lambda rs, n, E: rs.permutation(n)),
    ('unused_cameras', 256, 32, 4, 64, lambda rs, n, E: rs.randint(0, 8, n) * 8),
    ('E1000_100_frames', 4096, 32, 4, 1000, lambda rs, n, E: rs.randint(0, 100, n)),
    ('E1000_100_frames_G1', 4096, 32, 1, 1000, lambda rs, n, E: rs.randint(0, 100, n)),
    ('G1_small', 256, 32, 1, 12, lambda rs, n, E: rs.randint(0, E, n)),
    ('training_shape_11_frames', 4096, 32, 4, 1000, lambda rs, n, E: rs.randint(0, 11, n)),
    ('training_shape_one_camera', 4096, 32, 4, 1000, lambda rs, n, E: np.full(n, 999)),
    ('odd_samples', 300, 20, 3, 9, lambda rs, n, E: rs.randint(0, E, n)),
]


def _grad_problem(case, seed=0):
    name, n, S, G, E, assign = case
    rs = np.random.RandomState(seed + n + G)
    d_hz = round_bf16((rs.randn(n * S, 128) * 0.01 * (rs.rand(n * S, 128) < 0.5)).astype(np.float32))   # (ReLU-masked, like the real one)
    wb = round_bf16((rs.randn(288, 128) / 17).astype(np.float32))
    wb[283 + G:] = 0
    return dict(n=n, S=S, G=G, E=E, d_hz=d_hz, wb=wb, cam=np.asarray(assign(rs, n, E), np.int64))


def grad_case_error(M, case, stride=1):
    """(max |err| / sum |products| over the entries with work, the kernel's g_embed, the float64 one) for one case"""
    P = _grad_problem(case)
    cam = P['cam'] if stride == 1 else np.stack([P['cam'], P['cam'] * 0 + 3, P['cam'] * 0 + 1], -1)
    g = torch.full((P['E'], P['G']), float('nan'), device=dev())
    M.glo_backward(bf(P['d_hz']), P['n'], P['S'], bf(P['wb']), I32(cam), g)
    ref, scale = R.embed_grad_from_dhz(P['d_hz'], P['wb'], P['cam'], P['S'], P['E'], P['G'])
    got = N(g).astype(np.float64)
    used = np.zeros(P['E'], bool)
    used[P['cam']] = True
    assert (got[~used] == 0.0).all() and not np.signbit(got[~used]).any()           # rows without a ray: exactly +0.0
    err = np.abs(got - ref)[used] / scale[used]
    return float(err.max()), got, ref


@pytest.mark.parametrize('case', GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_embedding_gradient_equals_float64_on_the_same_operands(M, case):
    err, got, ref = grad_case_error(M, case)
    print('glo_backward %s: max |err| / sum |products| = %.3e' % (case[0], err))
    assert np.isfinite(got).all()
    assert err <= GRAD_ERR_GATE, (case[0], err)
    err3, got3, _ = grad_case_error(M, case, stride=3)                               # the pix [n, 3] form: same bits
    np.testing.assert_array_equal(got3, got)


@pytest.mark.parametrize('case', [GRAD_CASES[2], GRAD_CASES[3]], ids=['unused_cameras', 'E1000_100_frames'])
def test_embedding_gradient_is_deterministic_and_owns_its_output(M, case):
    P = _grad_problem(case)
    d_hz, wb, cam = bf(P['d_hz']), bf(P['wb']), I32(P['cam'])
    outs = []
    for fill in (0.0, float('nan'), 123.0):
        g = torch.full((P['E'], P['G']), fill, device=dev())
        M.glo_backward(d_hz, P['n'], P['S'], wb, cam, g, partial=torch.full((4 * P['n'],), fill, device=dev()))
        outs.append(N(g.view(torch.int32)))
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])


# ---------------------------------------------------------------------------------------- gradients through the MLP
def _nerf_params(rs, G):
    from oracle import mip360_oracle as O
    params = O.init_mlp_params(O.NERF_CFG, rs)
    D = O.NERF_CFG['net_depth']
    lim = np.sqrt(6.0 / (283 + G))
    params[D + 2] = (rs.uniform(-lim, lim, (283 + G, 128)).astype(np.float32), params[D + 2][1])
    return [(w, (rs.randn(*b.shape) * 0.05).astype(np.float32)) for w, b in params]


@pytest.mark.parametrize('fm', [True, False], ids=['fm', 'row_major'])
def test_mlp_gradients_with_embeddings_match_float64_autograd(M, fm):
    """One forward / backward of the NerfMLP with G = 4 (the fused fm path and the row-major fallback): the embedding's gradient,
    the view layer's kernel gradient (all 287 rows) and the bottleneck head's, against float64 autograd of the reference through
    the trunk head and the whole view branch on the kernel's own bf16 trunk activation and bf16-rounded parameters.  Gates: the
    two of test_gpu_mip360.py::test_mlp_backward_matches_oracle for every kernel gradient (same arithmetic class: bf16 operands
    of the same GEMMs, float32 accumulation) -- relative Frobenius error 3e-2 against float64 that rounds to bf16 where the
    kernels store a bf16 operand (the reference's round_like_kernels), 0.25 against float64 that rounds nothing in between.
    Measured: 2.5e-2 .. 3.9e-2 without the intermediate rounding (the embedding 2.7e-2)."""
    from oracle import mip360_oracle as O
    from tests.test_gpu_mip360 import _rays
    rs = np.random.RandomState(13)
    n, S, G, E = 16, 32, 4, 6
    rows, W, D = n * S, 1024, 8
    params = _nerf_params(rs, G)
    tm = M.TrainableMLP(params, M.NERF_CFG, dev())
    rays = _rays(rs, n)
    s = np.sort(rs.rand(n, S + 1), -1).astype(np.float32)
    _, s_to_t = O.construct_ray_warps('reciprocal', rays['near'], np.full((n, 1), 30., np.float32))
    tdist = s_to_t(s).astype(np.float32)
    basis = T(O.pos_basis_t())
    embed = (rs.randn(E, G) * 0.5).astype(np.float32)
    cam = rs.randint(0, E, n)
    embed_t, cam_t = T(embed), I32(cam)
    if fm:
        buf = M.fm_buffer(rows, W + 512, dev())
        M.cast_encode_fm(T(tdist), T(rays['origins']), T(rays['directions']), T(rays['radii']), basis, buf, W, W + 512)
        density, rgb, saved = M.mlp_forward_train_fm(tm, buf, rows, T(rays['viewdirs']), n, S, glo=(embed_t, cam_t))
        x_fm, x_col0, x_ld, x_k = saved['trunk']
        trunk = N(M.from_fm(x_fm, rows, x_k, ld=x_ld, col0=x_col0))
    else:
        buf = torch.empty(rows, W + 512, dtype=torch.bfloat16, device=dev())
        M.cast_encode(T(tdist), T(rays['origins']), T(rays['directions']), T(rays['radii']), basis, out=buf[:, W:], ld=W + 512)
        density, rgb, saved = M.mlp_forward_train(tm, buf, rows, T(rays['viewdirs']), n, S, glo=(embed_t, cam_t))
        trunk = N(saved['trunk'][0][:, :saved['trunk'][1]])
    g_d = np.zeros((n, S), np.float32)
    g_c = rs.randn(n, S, 3).astype(np.float32)
    g_embed = torch.full((E, G), float('nan'), device=dev())
    M.mlp_backward(tm, saved, rows, T(g_d).reshape(-1), T(g_c).reshape(-1, 3), [None, None], glo_grad=[g_embed, None])
    # float64 autograd: trunk head + view branch
    r64 = lambda a: torch.from_numpy(round_bf16(np.asarray(a, np.float32)).astype(np.float64))
    rel = lambda a, b: np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)
    got_e = N(g_embed).astype(np.float64)
    used = np.zeros(E, bool)
    used[cam] = True
    assert (got_e[~used] == 0).all()
    assert tuple(tm.kernel(D + 2, tm.grads).shape) == (283 + G, 128)
    dirs = round_bf16(R.dir_features(rays['viewdirs']).numpy().astype(np.float32))
    for rounded, gate in ((True, 3e-2), (False, 0.25)):
        w_b, w1, w2 = (r64(params[t][0]).requires_grad_(True) for t in (D + 1, D + 2, D + 3))
        e64 = r64(embed).requires_grad_(True)
        bott = R.trunk_head(trunk, w_b, params[D + 1][1], round_like_kernels=rounded)
        x = R.view_input(bott, np.repeat(dirs, S, 0), e64, np.repeat(cam, S))
        ref_rgb, _ = R.view_branch(x, w1, params[D + 2][1], w2, params[D + 3][1], round_like_kernels=rounded)
        np.testing.assert_allclose(N(rgb), ref_rgb.detach().numpy(), rtol=0, atol=1.5e-2)
        (ref_rgb * torch.from_numpy(g_c.reshape(-1, 3).astype(np.float64))).sum().backward()
        figures = {'embed': rel(got_e, e64.grad.numpy()),
                   'view kernel': rel(N(tm.kernel(D + 2, tm.grads)).astype(np.float64), w1.grad.numpy()),
                   'view kernel rows 283..286': rel(N(tm.kernel(D + 2, tm.grads)).astype(np.float64)[283:], w1.grad.numpy()[283:]),
                   'bottleneck kernel': rel(N(tm.kernel(D + 1, tm.grads)).astype(np.float64), w_b.grad.numpy())}
        print('relative Frobenius errors (%s, reference %s): %s'
              % ('fm' if fm else 'row-major', 'rounding like the kernels' if rounded else 'without intermediate rounding', figures))
        for k, v in figures.items():
            assert v < gate, (k, v, gate)


# ------------------------------------------------------------------------------------------------------- the trainer
class _CountingLib(object):
    def __init__(self, lib):
        self._lib_, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib_, name)
        if 'glo' in name and name != 'mip360_glo_revision':
            self.calls.append(name)
        return fn


def _toy_batch(n, seed=5):
    from tests.test_gpu_mip360 import _rays
    rs = np.random.RandomState(seed)
    rays = {k: T(v) for k, v in _rays(rs, n).items()}
    gt = T(rs.rand(n, 3).astype(np.float32))
    sup = T((0.5 + rs.rand(n)).astype(np.float32))
    jit = [[T(np.random.RandomState(10 * s_ + l).rand(n).astype(np.float32)) for l in range(3)] for s_ in range(3)]
    return rays, gt, sup, jit, I32(rs.randint(0, 7, n))


def test_zero_features_is_the_model_without_embeddings(M, monkeypatch):
    from oracle import mip360_oracle as O
    rays, gt, sup, jit, cam = _toy_batch(64)
    counting = _CountingLib(M.lib())
    monkeypatch.setattr(M, '_lib', counting)
    out = []
    for kw, cam_arg in ((dict(), None), (dict(num_glo_features=0, num_glo_embeddings=1000), cam)):
        prs = np.random.RandomState(7)
        tr = M.Mip360Trainer(O.init_mlp_params(O.PROP_CFG, prs), O.init_mlp_params(O.NERF_CFG, prs), dev(), max_steps=1000, **kw)
        hist = [N(tr.train_step(rays, gt, sup, jitter01=jit[s_], cam_idx=cam_arg)) for s_ in range(3)]
        tr.flush()
        assert tr.glo is None and 'glo' not in tr.state_dict()
        out.append((np.stack(hist), N(tr.prop.flat), N(tr.nerf.flat), N(tr.nerf.mu), N(tr.nerf.nu)))
    assert counting.calls == []
    for a, b in zip(*out):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))
    # ... and with features the same wrapper sees the three launches of a step
    prs = np.random.RandomState(7)
    tr = M.Mip360Trainer(O.init_mlp_params(O.PROP_CFG, prs), _nerf_params(prs, 4), dev(), max_steps=1000, num_glo_features=4,
                         num_glo_embeddings=7)
    with pytest.raises(M.Mip360Error, match='cam_idx'):
        tr.train_step(rays, gt, sup, jitter01=jit[0])
    tr.train_step(rays, gt, sup, jitter01=jit[0], cam_idx=cam)
    tr.flush()
    assert counting.calls == ['mip360_dir_glo_encode', 'mip360_glo_backward']
    with pytest.raises(M.Mip360Error, match='287 input rows'):
        M.Mip360Trainer(O.init_mlp_params(O.PROP_CFG, prs), O.init_mlp_params(O.NERF_CFG, prs), dev(), num_glo_features=4)


def test_embedding_joins_the_nerf_mlp_clipping_group_and_adam(M):
    """The clipping norm is the norm over the NerfMLP's tensors and the embedding's gradient together (upstream clips one tree);
    rows of cameras without a ray have zero gradient and zero moments after the first step, so they stay bit-identical.  (The
    rows in use move by lr g / (|g| + eps) with the CLIPPED g, far below lr on this toy batch whose norm is large: only that some
    component moves, and none by more than lr, is asserted -- as test_gpu_mip360.py does for the NerfMLP.)"""
    from oracle import mip360_oracle as O
    rays, gt, sup, jit, cam = _toy_batch(64)
    prs = np.random.RandomState(7)
    tr = M.Mip360Trainer(O.init_mlp_params(O.PROP_CFG, prs), _nerf_params(prs, 4), dev(), max_steps=1000, num_glo_features=4,
                         num_glo_embeddings=12)
    before = N(tr.glo.embed).copy()
    tr.train_step(rays, gt, sup, jitter01=jit[0], cam_idx=cam)
    tr.flush()
    g_nerf, g_e = N(tr.nerf.grads).astype(np.float64), N(tr.glo.grads).astype(np.float64)
    assert np.abs(g_e[:7]).min() > 0 and (g_e[7:] == 0).all()
    norm = np.sqrt((g_nerf ** 2).sum() + (g_e ** 2).sum())
    clip = N(tr.clip)
    np.testing.assert_allclose(clip[0, 1], norm, rtol=1e-4)
    np.testing.assert_allclose(clip[0, 0], min(1.0, 0.001 / (np.finfo(np.float32).eps + norm)), rtol=1e-4)
    after = N(tr.glo.embed)
    np.testing.assert_array_equal(after[7:], before[7:])
    delta = np.abs(after[:7] - before[:7])
    assert delta.max() > 0 and delta.max() <= M.learning_rate(0, max_steps=1000) * 1.001


# ------------------------------------------------------------------------------------- it does what it is for
GAIN_STEPS, GAIN_TAIL = 400, 50


def gain_scene_curves(tmp, G, steps=GAIN_STEPS, seed=0):
    """The 12-frame scene of tests/test_mip360_scene.py::write_scene whose training frames are multiplied by a per-frame, per-channel
    colour gain (uniform in [0.6, 1.4], RandomState(1234), clipped to bytes), trained `steps` steps of 1024 rays with the CLI's
    trainer for the Config.  Returns (data-loss curve, trainer, number of train frames)."""
    from outdoor_nerf_depth_amd import mip360_data as D
    from outdoor_nerf_depth_amd import mip360_train as TR
    from tests.test_mip360_scene import write_scene
    data = os.path.join(str(tmp), 'scene')
    if not os.path.isdir(data):
        write_scene(data, n_frames=12, H=32, W=40)
    cfg = D.parse_gin(bindings=["Config.data_dir = '%s'" % data, "Config.depth_sup_type = 'mono_crop'", 'Config.max_steps = %d' % steps,
                                'Config.lr_delay_steps = 0', 'Config.batch_size = 1024', 'Model.num_glo_features = %d' % G,
                                'Model.num_glo_embeddings = 16'])
    scene = D.Scene(cfg)
    gains = np.random.RandomState(1234).uniform(0.6, 1.4, (len(scene.names), 1, 1, 3))
    scene.images = np.clip(np.round(scene.images.astype(np.float64) * gains), 0, 255).astype(np.uint8)
    train = scene.device_frames('train', dev())
    F = train['cams'].shape[0]
    tr = TR.make_trainer(cfg, dev(), n_train_frames=F)
    curve = []
    for counter in range(steps):
        b = _m().sample_batch(train['cams'], train['rgb_u8'], train['depth_sup'], seed, counter, 1024, scene.near, scene.far)
        curve.append(tr.train_step(b['rays'], b['rgb'], b['depth_sup'], jitter01=list(b['jitter01']),
                                   cam_idx=b['pix'] if G else None)[1:2].clone())
    tr.flush()
    return torch.cat(curve).cpu().numpy().astype(np.float64), tr, F


def test_embeddings_absorb_per_frame_colour_gains(M, tmp_path):
    c4, tr4, F = gain_scene_curves(tmp_path, 4)
    c0, tr0, _ = gain_scene_curves(tmp_path, 0)
    assert tr0.glo is None and np.isfinite(c4).all() and np.isfinite(c0).all()
    final4, final0 = c4[-GAIN_TAIL:].mean(), c0[-GAIN_TAIL:].mean()
    noise = max(c4[-GAIN_TAIL:].std(), c0[-GAIN_TAIL:].std()) / np.sqrt(GAIN_TAIL)
    print('data loss, mean of the last %d of %d steps: G=4 %.6f, G=0 %.6f, gap %.6f, standard error %.6f'
          % (GAIN_TAIL, GAIN_STEPS, final4, final0, final0 - final4, noise))
    # (a) the rows of the frames in use moved and differ from one another; the others never received a gradient: moments zero,
    #     value exactly the initial one
    e = N(tr4.glo.embed)
    assert F == 11
    mu, nu = N(tr4.glo.mu), N(tr4.glo.nu)
    assert (mu[F:] == 0).all() and (nu[F:] == 0).all()
    first = gain_first_embed(tmp_path)
    np.testing.assert_array_equal(e[F:], first[F:])
    assert (np.abs(e[:F] - first[:F]).max(-1) > 1e-3).all()
    dist = np.linalg.norm(e[:F, None] - e[None, :F], axis=-1) + np.eye(F)
    assert dist.min() > 1e-3
    # (b) the embeddings lower the training data loss
    assert final0 - final4 > TRAIN_GAP_GATE, (final0, final4)


def gain_first_embed(tmp):
    """the embedding table make_trainer draws for the Config of gain_scene_curves(G = 4), before any step"""
    from outdoor_nerf_depth_amd import mip360_data as D
    from outdoor_nerf_depth_amd import mip360_train as TR
    cfg = D.parse_gin(bindings=['Config.max_steps = %d' % GAIN_STEPS, 'Model.num_glo_features = 4', 'Model.num_glo_embeddings = 16'])
    return N(TR.make_trainer(cfg, dev()).glo.embed)


# ------------------------------------------------------------------------------------------------ checkpoints, CLIs
def test_state_dict_round_trip_and_mismatches(M):
    from oracle import mip360_oracle as O
    rays, gt, sup, jit, cam = _toy_batch(64)

    def trainer(G, E=12):
        prs = np.random.RandomState(7)
        kw = dict(num_glo_features=G, num_glo_embeddings=E) if G else {}
        return M.Mip360Trainer(O.init_mlp_params(O.PROP_CFG, prs), _nerf_params(prs, G), dev(), max_steps=1000, **kw)
    full = trainer(4)
    for s_ in range(2):
        full.train_step(rays, gt, sup, jitter01=jit[s_], cam_idx=cam)
        if s_ == 0:
            state = full.state_dict()
    assert state['glo']['num_glo_features'] == 4 and state['glo']['num_glo_embeddings'] == 12
    assert tuple(state['glo']['glo_embed'].shape) == (12, 4)
    resumed = trainer(4)
    resumed.load_state_dict(state)
    resumed.train_step(rays, gt, sup, jitter01=jit[1], cam_idx=cam)
    full.flush(), resumed.flush()
    for a, b in ((full.nerf.flat, resumed.nerf.flat), (full.prop.flat, resumed.prop.flat), (full.glo.embed, resumed.glo.embed),
                 (full.glo.mu, resumed.glo.mu), (full.glo.nu, resumed.glo.nu)):
        assert torch.equal(a, b)
    plain = trainer(0)
    old = plain.state_dict()
    assert set(old) == {'step', 'prop', 'nerf'}                    # what a checkpoint written before the embeddings holds
    trainer(0).load_state_dict(old)
    with pytest.raises(M.Mip360Error, match=r'written with Model.num_glo_features = 0.*this trainer has num_glo_features = 4'):
        trainer(4).load_state_dict({k: v for k, v in old.items()})
    with pytest.raises(M.Mip360Error, match=r'num_glo_features = 4.*this trainer has num_glo_features = 0'):
        plain.load_state_dict(state)
    with pytest.raises(M.Mip360Error, match=r'num_glo_embeddings = 12.*num_glo_embeddings = 20'):
        trainer(4, 20).load_state_dict(state)


def test_cli_trains_resumes_and_evaluates_with_embeddings(tmp_path):
    """mip360_train with --gin_bindings "Model.num_glo_features = 4": checkpoints with the table, a test render; a run resumed
    from step 30 ends bit-identical to the uninterrupted one; mip360_eval writes the metric files it writes without embeddings;
    a checkpoint without embeddings is refused by a config with them."""
    import shutil
    from tests.test_gpu_mip360_app import _bindings, _run
    from tests.test_mip360_scene import write_scene
    data, ckpt = tmp_path / 'scene', tmp_path / 'run'
    write_scene(str(data), n_frames=12, H=32, W=40)
    glo = ['Model.num_glo_features = 4', 'Model.num_glo_embeddings = 32']
    _run('mip360_train', _bindings(data, ckpt, glo))
    for s in (1, 30, 60):
        assert (ckpt / ('checkpoint_%d' % s)).is_file()
    for f in ('color_000.png', 'depth_000.png', 'metric_psnr_60.txt', 'metric_rmse_60.txt', 'metric_absrel_60.txt'):
        assert (ckpt / 'test_preds_60' / f).is_file(), f
    a = torch.load(str(ckpt / 'checkpoint_60'), map_location='cpu')
    assert a['trainer']['glo']['num_glo_features'] == 4 and tuple(a['trainer']['glo']['glo_embed'].shape) == (32, 4)
    assert a['trainer']['nerf']['params'].numel() == sum(i * o + o for i, o in _m().mlp_shapes(_m().NERF_CFG, 4))
    run2 = tmp_path / 'resumed'
    run2.mkdir()
    shutil.copy(str(ckpt / 'checkpoint_30'), str(run2 / 'checkpoint_30'))
    out = _run('mip360_train', _bindings(data, run2, glo))
    assert 'Resuming from' in out
    b = torch.load(str(run2 / 'checkpoint_60'), map_location='cpu')
    assert a['counter'] == b['counter'] and a['trainer']['step'] == b['trainer']['step'] == 60
    for mlp in ('prop', 'nerf'):
        for k in ('params', 'mu', 'nu'):
            assert torch.equal(a['trainer'][mlp][k], b['trainer'][mlp][k]), (mlp, k)
    for k in ('glo_embed', 'mu', 'nu'):
        assert torch.equal(a['trainer']['glo'][k], b['trainer']['glo'][k]), k
    first = torch.load(str(ckpt / 'checkpoint_1'), map_location='cpu')
    assert not torch.equal(first['trainer']['glo']['glo_embed'][:11], a['trainer']['glo']['glo_embed'][:11])
    assert torch.equal(first['trainer']['glo']['glo_embed'][11:], a['trainer']['glo']['glo_embed'][11:])      # 11 train frames
    _run('mip360_eval', _bindings(data, ckpt, glo + ["Config.eval_suffix = 'x'"]))
    d = ckpt / 'test_eval_preds_x'
    for f in ('color_000.png', 'depth_000.png', 'absrel_000.npy', 'distance_mean_000.tiff', 'distance_median_000.tiff', 'acc_000.tiff',
              'metric_psnr_60.txt', 'metric_rmse_60.txt', 'metric_absrel_60.txt', 'metric_disparity_mean_mse_60.txt',
              'metric_disparity_median_mse_60.txt'):
        assert (d / f).is_file(), f
    # a run without embeddings cannot continue a checkpoint with them
    import subprocess
    import sys
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    p = subprocess.run([sys.executable, '-m', 'outdoor_nerf_depth_amd.mip360_eval'] + _bindings(data, ckpt), capture_output=True, text=True,
                       env=env, timeout=600)
    assert p.returncode != 0 and 'written with Model.num_glo_features = 4' in p.stderr and 'num_glo_features = 0' in p.stderr


def _m():
    from outdoor_nerf_depth_amd import mip360
    return mip360
