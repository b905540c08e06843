"""GPU tests of the ray-side kernels of the MipNeRF-360 path at their edges, one by one through the C ABI, against the float64
restatements of tests/mip360_rays_reference.py (R) and inside the bounds that module derives (tests/test_mip360_rays_reference.py shows
on the CPU that float32 numpy twins pass them on these very inputs and that mutated twins do not):

* mip360_resample: m_in around the 64-lane rounds and at the LDS rows' capacity, ns at both ends, 1 ... 37 rays (four per block), the
  four dilations and two paddings, no / zero / largest / random jitter, six input families -- every sdist edge inside the cdf-space
  envelope, monotone, inside the domain, tdist against s_to_t of the kernel's own sdist, two runs bit-identical;
* mip360_cast_encode: 1 ... 193 rows (3 per wave, 12 per block), float32 and bf16 through the staged, the unstaged and the
  fragment-major stores, out of views of larger sentinel-filled tensors;
* mip360_distance_percentiles: S = 1 ... 62, tied cdf values, sums below / at / above 1, all-zero rays -- within one float32 ulp;
* mip360_dir_encode: widths 27 and 32 at column offsets 0, 8 and 5;
* mip360_frame_rays / mip360_sample_batch: ray counts around the 256-ray blocks, bit-equal to the whole-frame call.

Every output buffer lies between sentinels; every output is asserted finite.  The worst ratio per kernel is printed (pytest -s)."""
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from oracle import mip360_oracle as O                                    # noqa: E402
from tests import mip360_rays_reference as R                             # noqa: E402
from tests.test_gpu_mip360 import T, dev                                 # noqa: E402
from tests.test_gpu_mip360_app import GOLDEN, golden_cams, _frames       # noqa: E402

SENTINEL = 7.0
GUARD = 64
WORST = {}


@pytest.fixture(scope='module')
def M():
    dev()
    from outdoor_nerf_depth_amd import mip360
    return mip360


def call(M, name, *args):
    M._check(getattr(M.lib(), name)(M._stream(), *args), name)


def note(name, value):
    WORST[name] = max(WORST.get(name, 0.0), float(value))
    return float(value)


class Guarded(object):
    """a device buffer [GUARD sentinels | shape | GUARD sentinels] and the view of its middle"""

    def __init__(self, shape, dtype=torch.float32, lead=GUARD):
        self.size = int(np.prod(shape))
        self.lead = lead
        self.buf = torch.full((lead + self.size + GUARD,), SENTINEL, dtype=dtype, device=dev())
        self.view = self.buf[lead:lead + self.size].view(*shape)

    def intact(self):
        return bool((self.buf[:self.lead] == SENTINEL).all()) and bool((self.buf[self.lead + self.size:] == SENTINEL).all())

    def host(self):
        out = self.view.cpu().numpy() if self.view.dtype != torch.bfloat16 else self.view.float().cpu().numpy()
        assert np.isfinite(out).all()
        return out


def bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------------------------ resampling
def _resample(M, c):
    n, m, ns = c['n'], c['m'], c['ns']
    so, to = Guarded((n, ns + 1)), Guarded((n, ns + 1))
    jit = None if c['jit'] is None else T(c['jit'].reshape(-1))
    sd, w, near, far = T(c['sd']), T(c['w']), T(c['near'].reshape(-1)), T(c['far'].reshape(-1))
    call(M, 'mip360_resample', n, m, M._p(sd), M._p(w), float(c['dilation']), float(R.ANNEAL), float(c['padding']), ns, M._p(jit),
         0.0, 1.0, M._p(near), M._p(far), M._p(so.view), M._p(to.view))
    assert so.intact() and to.intact()
    return so.host(), to.host()


@pytest.mark.parametrize('m', R.RESAMPLE_M)
def test_resample_edges_inside_the_cdf_envelope(M, m):
    for c in R.resample_cases(m):
        b = R.resample_bounds(c['sd'], c['w'], c['dilation'], R.ANNEAL, c['padding'], c['ns'], c['jit'])
        got_s, got_t = _resample(M, c)
        r = R.envelope_ratio(got_s, b['lo'], b['want'], b['hi'])
        where = (c['m'], c['ns'], c['n'], c['dilation'], c['padding'], c['jitter'], c['families'][int(np.argmax(r.max(-1)))])
        note('resample, off the domain ends', np.where((got_s > 0) & (got_s < 1), r, 0).max())  # (an edge clipped onto 0 or 1 sits ON its bound: ratio 1)
        assert note('resample', r.max()) <= 1.0, where + (float(r.max()), float(R.excess(got_s, b['lo'], b['hi']).max()))
        assert (np.diff(got_s) >= 0).all(), where
        assert got_s[:, 0].min() >= 0.0 and got_s[:, -1].max() <= 1.0, where
        _, s_to_t = O.construct_ray_warps('reciprocal', c['near'], c['far'])
        np.testing.assert_allclose(1.0 / got_t, 1.0 / s_to_t(got_s), rtol=2e-6, atol=1e-9, err_msg=str(where))
        again_s, again_t = _resample(M, c)
        assert np.array_equal(got_s.view(np.uint32), again_s.view(np.uint32)) and np.array_equal(got_t.view(np.uint32), again_t.view(np.uint32))


def test_resample_refuses_sizes_beyond_its_lds_rows(M):
    z = torch.zeros(4 * 200, device=dev())
    args = lambda m, ns: (1, m, M._p(z), M._p(z), 0.0, 1.0, 0.0, ns, None, 0.0, 1.0, M._p(z), M._p(z), M._p(z), M._p(z))
    for m, ns, words in ((129, 64, '1 <= m_in <= 128'), (64, 1, '2 <= num_samples <= 64'), (64, 65, '2 <= num_samples <= 64')):
        with pytest.raises(M.Mip360Error, match=re.escape('mip360_resample: requirement failed: ' + words)):
            call(M, 'mip360_resample', *args(m, ns))
    assert not bool(z.any())


# ------------------------------------------------------------------------------------------------------------ featurisation
_ENCODE = {}


def _encode_inputs(n, S):
    """inputs, float64 reference and bounds of one (n, S), computed once and shared"""
    if (n, S) not in _ENCODE:
        basis = O.pos_basis_t()
        case = R.encode_case(n, S)
        ref = R.encode_reference(*case, basis)
        b32 = R.encode_bound(ref, *R.encode_deltas(*case, basis), R.in_todays_domain(*case))
        _ENCODE[(n, S)] = dict(case=case, dev=[T(a) for a in case] + [T(basis)], ref=ref, b32=b32, b16=R.encode_bound_bf16(ref, b32))
    return _ENCODE[(n, S)]


def _window(rows, ld, dtype, byte_offset=0):
    """rows of `ld` elements inside a sentinel-filled allocation, one row of sentinels before and after: (flat buffer, [rows, ld] view
    that starts `byte_offset` bytes into the second row)"""
    item = 2 if dtype == torch.bfloat16 else 4
    off = byte_offset // item
    flat = torch.full(((rows + 2) * ld + off,), SENTINEL, dtype=dtype, device=dev())
    view = flat[ld + off:ld + off + rows * ld].view(rows, ld)
    assert view.data_ptr() % 16 == (ld * item + byte_offset) % 16
    return flat, view


def _encode_into(M, e, dtype, ld, byte_offset=0):
    rows = e['ref']['want'].shape[0]
    flat, view = _window(rows, ld, dtype, byte_offset)
    M.cast_encode(*e['dev'], out=view, ld=ld)
    assert bool((flat[:view.storage_offset()] == SENTINEL).all()) and bool((flat[view.storage_offset() + rows * ld:] == SENTINEL).all())
    pad_to = min(ld, 512)
    if pad_to > 504:
        assert not bool(view[:, 504:pad_to].any())                        # the K padding of the next layer
    if ld > 512:
        assert bool((view[:, 512:] == SENTINEL).all())                    # nothing outside the window is touched
    return view[:, :504]


@pytest.mark.parametrize('n,S', R.ENCODE_ROWS)
def test_cast_encode_float32_rows(M, n, S):
    e = _encode_inputs(n, S)
    for ld in (504, 512, 520):
        got = _encode_into(M, e, torch.float32, ld).cpu().numpy()
        assert np.isfinite(got).all()
        r = R.err_ratio(got, e['ref']['want'], e['b32'])
        assert note('cast_encode float32', r.max()) <= 1.0, (ld, np.unravel_index(int(np.argmax(r)), r.shape), float(r.max()))


@pytest.mark.parametrize('n,S', R.ENCODE_ROWS)
def test_cast_encode_bf16_staged_and_unstaged_rows(M, n, S):
    """staged: ld >= 512, ld % 8 == 0 and a 16-byte aligned base; everything else takes the 2-byte stores -- ld = 504 (< 512), ld = 516
    (not a multiple of 8), ld = 768 from a base 8 bytes off alignment.  Same bits either way."""
    e = _encode_inputs(n, S)
    first = None
    for ld, byte_offset in ((512, 0), (768, 0), (504, 0), (516, 0), (768, 8)):
        view = _encode_into(M, e, torch.bfloat16, ld, byte_offset)
        got = view.float().cpu().numpy()
        assert np.isfinite(got).all()
        r = R.err_ratio(got, e['ref']['want'], e['b16'])
        assert note('cast_encode bf16', r.max()) <= 1.0, (ld, byte_offset, np.unravel_index(int(np.argmax(r)), r.shape), float(r.max()))
        first = bits(view) if first is None else first
        assert np.array_equal(bits(view), first), (ld, byte_offset)


@pytest.mark.parametrize('n,S', R.ENCODE_FM_ROWS)
def test_cast_encode_fragment_major_has_the_bits_of_the_staged_rows(M, n, S):
    e = _encode_inputs(n, S)
    rows = n * S
    staged = torch.full((rows, 512), SENTINEL, dtype=torch.bfloat16, device=dev())
    M.cast_encode(*e['dev'], out=staged, ld=512)
    r = R.err_ratio(staged[:, :504].float().cpu().numpy(), e['ref']['want'], e['b16'])
    assert note('cast_encode bf16', r.max()) <= 1.0
    for ld, col0 in ((512, 0), (768, 256)):
        got, want = (torch.full((rows * ld + GUARD,), SENTINEL, dtype=torch.bfloat16, device=dev()) for _ in range(2))
        M.cast_encode_fm(*e['dev'], got, col0, ld)
        M.to_fm(staged, out=want, ld=ld, col0=col0)
        assert np.array_equal(bits(got), bits(want)), (ld, col0)
        assert bool((got[rows * ld:] == SENTINEL).all())
        if col0:
            assert bool((got == SENTINEL).any())                          # the columns before col0 stay as they were
        assert np.array_equal(bits(M.from_fm(got, rows, 512, ld=ld, col0=col0)), bits(staged))


# ------------------------------------------------------------------------------------------------------------ percentiles
@pytest.mark.parametrize('S', R.PCT_S)
def test_distance_percentiles_within_one_ulp(M, S):
    for i, n in enumerate(R.PCT_N):
        for far in (1e3, 1e6):
            tdist, w, t_far = R.percentile_case(S, n, far, i)
            out = Guarded((n, 3))
            td, wd, fd = T(tdist), T(w), T(t_far.reshape(-1))
            call(M, 'mip360_distance_percentiles', n, S, M._p(td), M._p(wd), M._p(fd), M._p(out.view))
            assert out.intact()
            want = R.percentile_reference(tdist, w, t_far)
            r = R.err_ratio(out.host(), want, R.percentile_bound(want))
            assert note('distance_percentiles', r.max()) <= 1.0, (S, n, far, R.PCT_FAMILIES[(i + int(np.argmax(r.max(-1)))) % 6], float(r.max()))


def test_distance_percentiles_refuses_more_edges_than_lanes(M):
    z = torch.zeros(256, device=dev())
    for S in (63, 64):
        with pytest.raises(M.Mip360Error, match=re.escape('mip360_distance_percentiles: requirement failed: n > 0, 1 <= S <= 62 (S + 2 edges in one wave)')):
            call(M, 'mip360_distance_percentiles', 1, S, M._p(z), M._p(z), M._p(z), M._p(z))
    assert not bool(z.any())


# ------------------------------------------------------------------------------------------------------------ direction features
@pytest.mark.parametrize('n,S', R.DIR_SHAPES)
def test_dir_encode_columns_zero_fill_and_sentinels(M, n, S):
    v = R.dir_case(n)
    want = np.repeat(R.dir_reference(v), S, 0)
    vd = T(v)
    for width in R.DIR_WIDTH:
        for col0 in R.DIR_COL0:
            ld = col0 + width + 3
            out = Guarded((n * S, ld), torch.bfloat16)
            call(M, 'mip360_dir_encode', n, S, M._p(vd), M._p(out.view), ld, col0, width)
            assert out.intact()
            got = out.host()
            r = R.err_ratio(got[:, col0:col0 + 27], want, R.dir_bound(want))
            assert note('dir_encode', r.max()) <= 1.0, (width, col0, float(r.max()))
            assert not got[:, col0 + 27:col0 + width].any()               # the zero fill: columns 27 ... width - 1
            assert (got[:, :col0] == SENTINEL).all() and (got[:, col0 + width:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------ rays
RAY_KEYS = ('origins', 'directions', 'viewdirs', 'radii', 'near', 'far')


def _ray_buffers(n):
    return {k: Guarded((n, 3 if k in RAY_KEYS[:3] else 1)) for k in RAY_KEYS}


@pytest.fixture(scope='module')
def frames(M):
    z = np.load(GOLDEN)
    cams = torch.from_numpy(golden_cams(z)).to(dev())
    H, W = (int(v) for v in z['hw'])
    full = [{k: v.cpu().numpy() for k, v in M.frame_rays(cams, c, W, 0, H * W, 0.2, 1e6).items()} for c in range(cams.shape[0])]
    return cams, H, W, full


def test_frame_rays_around_the_block_size_equal_the_whole_frame(M, frames):
    cams, H, W, full = frames
    for c in range(cams.shape[0]):                                        # pinhole, simple_radial, opencv, rotated
        for n in (1, 255, 256, 257):
            for p0 in (0, W - 1, 17):
                out = _ray_buffers(n)
                call(M, 'mip360_frame_rays', M._p(cams), cams.shape[0], c, W, p0, n, 0.2, 1e6, *[M._p(out[k].view) for k in RAY_KEYS])
                for k in RAY_KEYS:
                    assert out[k].intact(), (c, n, p0, k)
                    assert np.array_equal(out[k].host().view(np.uint32), full[c][k][p0:p0 + n].view(np.uint32)), (c, n, p0, k)


@pytest.mark.parametrize('n', [1, 257])
@pytest.mark.parametrize('num_levels', [0, 3])
@pytest.mark.parametrize('with_gt', [False, True])
def test_sample_batch_around_the_block_size(M, frames, n, num_levels, with_gt):
    cams, H, W, full = frames
    F = cams.shape[0]
    rgb, sup, gt, rgb_d, sup_d, gt_d = _frames(dev(), F, H, W)
    out = _ray_buffers(n)
    col, s_out, g_out = Guarded((n, 3)), Guarded((n,)), Guarded((n,))
    pix = Guarded((n, 3), torch.int32)
    jit = Guarded((max(num_levels, 1), n))
    call(M, 'mip360_sample_batch', M._p(cams), F, H, W, 5, 11, n, M._p(rgb_d), M._p(sup_d), M._p(gt_d) if with_gt else None, 0.2, 1e6,
         num_levels, *[M._p(out[k].view) for k in RAY_KEYS], M._p(col.view), M._p(s_out.view), M._p(g_out.view) if with_gt else None,
         M._p(pix.view), M._p(jit.view) if num_levels else None)
    for g in list(out.values()) + [col, s_out, g_out, pix, jit]:
        assert g.intact()
    p = pix.host()
    c, x, y = p[:, 0], p[:, 1], p[:, 2]
    assert (c >= 0).all() and (c < F).all() and (x >= 0).all() and (x < W).all() and (y >= 0).all() and (y < H).all()
    for k in RAY_KEYS:
        want = np.stack([full[ci][k][yi * W + xi] for ci, xi, yi in zip(c, x, y)], 0)
        assert np.array_equal(out[k].host().view(np.uint32), want.view(np.uint32)), k
    assert np.array_equal(col.host(), np.float32(rgb[c, y, x] / 255.)) and np.array_equal(s_out.host(), sup[c, y, x])
    if with_gt:
        assert np.array_equal(g_out.host(), gt[c, y, x])
    else:
        assert bool((g_out.view == SENTINEL).all())                        # no depth_gt: gt_out is never written
    if num_levels:
        j = jit.host()
        assert (j >= 0).all() and (j < 1).all()
    else:
        assert bool((jit.view == SENTINEL).all())                          # no levels: the jitter buffer may be null and is not written
    # the first n rays of a larger draw are the same rays: a ray's draw depends on its index alone, not on the launch's size
    more = M.sample_batch(cams, rgb_d, sup_d, seed=5, counter=11, n=n + 300, near=0.2, far=1e6, depth_gt=gt_d if with_gt else None,
                          num_levels=num_levels)
    assert np.array_equal(more['pix'].cpu().numpy()[:n], p)


def test_zz_report_worst_ratios():
    """the worst |error| / bound per kernel over this module (DESIGN.md quotes them)"""
    for k in sorted(WORST):
        print('MI355X, worst ratio  %-24s %.3f' % (k, WORST[k]))
    assert all(v <= 1.0 for v in WORST.values())
