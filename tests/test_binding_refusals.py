"""What the six evaluator bindings (image_metrics, lpips, color_correct, depth_vis, depth_metrics, depth_consistency) share, held
from outside: every refusal's exception class and full text, the pending result's one read, and the workspace cache's two
eviction rules with the rule that a pending result keeps its workspace.  The expected strings were recorded from the bindings
while each still carried its own copy of the checks.

Not marked gpu: the refusals a host without a device reaches, the negative size queries and `Pending` on stand-in tensors.
Marked gpu: the refusals that need a device tensor, the cache, and non-contiguous inputs where a binding copies.  Every tensor
is at most [2, 16, 16, 3].
"""
import weakref

import numpy as np
import pytest
import torch

from outdoor_nerf_depth_amd import _ctypes_util as U
from outdoor_nerf_depth_amd import _lib as L
from outdoor_nerf_depth_amd import color_correct as CC
from outdoor_nerf_depth_amd import depth_consistency as DC
from outdoor_nerf_depth_amd import depth_metrics as DM
from outdoor_nerf_depth_amd import depth_vis as DV
from outdoor_nerf_depth_amd import image_metrics as IM
from outdoor_nerf_depth_amd import lpips as LP

gpu = pytest.mark.gpu


def refused(error, message, call, *args, **kw):
    with pytest.raises(error) as e:
        call(*args, **kw)
    assert type(e.value) is error and str(e.value) == message


def _weights():
    return object.__new__(LP.Weights)                     # passes lpips_u8's isinstance question; never packed


DV_NO_CPU = '%s: expected a CUDA/HIP float32 tensor (the depth pictures have no CPU path)'
DC_NO_CPU = '%s: expected a CUDA/HIP float32 tensor (the consistency check has no CPU path)'
# (id, call of one argument that stands in for every frame argument, error, text)
NO_DEVICE = [
    ('image_metrics', lambda x: IM.image_metrics_async(x, x), L.NerfppError,
     'gt_u8: expected a CUDA/HIP uint8 tensor (image_metrics has no CPU path)'),
    ('image_metrics_blocking', lambda x: IM.image_metrics(x, x), L.NerfppError,
     'gt_u8: expected a CUDA/HIP uint8 tensor (image_metrics has no CPU path)'),
    ('lpips', lambda x: LP.lpips_u8(x, x, _weights()), LP.LpipsError, 'gt_u8: expected a CUDA/HIP uint8 tensor (lpips_u8 has no CPU path)'),
    ('color_correct', lambda x: CC.color_correct_async(x, x), CC.ColorCorrectError,
     'img_f32: expected a CUDA/HIP torch.float32 tensor (color_correct has no CPU path)'),
    ('normal_equations', lambda x: CC.normal_equations(x, x), CC.ColorCorrectError,
     'img_f32: expected a CUDA/HIP torch.float32 tensor (color_correct has no CPU path)'),
    ('weighted_percentiles', lambda x: DV.weighted_percentiles_async(x, x, (50.,)), DV.DepthVisError, DV_NO_CPU % 'value'),
    ('minmax', lambda x: DV.minmax(x), DV.DepthVisError, DV_NO_CPU % 'value'),
    ('colorize_cmap', lambda x: DV.colorize_cmap_async(x, x), DV.DepthVisError, DV_NO_CPU % 'value'),
    ('minmax_colorize', lambda x: DV.minmax_colorize_async(x), DV.DepthVisError, DV_NO_CPU % 'value'),
    ('matte_rgb', lambda x: DV.matte_rgb_async(x, x), DV.DepthVisError, DV_NO_CPU % 'rgb'),
    ('coords_mod', lambda x: DV.coords_mod_async(x, x, x, x), DV.DepthVisError, DV_NO_CPU % 'origins'),
    ('mip360_suite', lambda x: DV.mip360_suite_async(x, x, x, x, x, x, x, x), DV.DepthVisError, DV_NO_CPU % 'acc'),
    ('mip360_depth_pair', lambda x: DV.mip360_depth_pair_async(x, x, x), DV.DepthVisError, DV_NO_CPU % 'acc'),
    ('depth_metrics', lambda x: DM.depth_metrics_async(x, x, 1.0), DM.DepthMetricsError,
     'pred: expected a CUDA/HIP float32 tensor (the depth metrics have no CPU path)'),
    ('depth_consistency_enqueue', lambda x: DC.enqueue(x, None, None, 0, DC.check_params()), DC.DepthConsError, DC_NO_CPU % 'depth'),
    ('depth_consistency_check', lambda x: DC.check_async(x, None, None), DC.DepthConsError, DC_NO_CPU % 'depth'),
]


@pytest.mark.parametrize('what', ['numpy', 'cpu_tensor'])
@pytest.mark.parametrize('name,call,error,message', NO_DEVICE, ids=[c[0] for c in NO_DEVICE])
def test_refuses_what_is_not_on_a_device(name, call, error, message, what):
    x = np.zeros((2, 4, 5), np.float32)
    refused(error, message, call, x if what == 'numpy' else torch.from_numpy(x))


def test_lpips_asks_for_its_weights_first():
    refused(LP.LpipsError, 'weights: expected lpips.Weights (load_weights), got NoneType', LP.lpips_u8, None, None, None)


def test_depth_consistency_answers_before_it_asks_for_a_device():
    """dtype, rank, contiguity, depth_out's shape and device, the overlap: all on host tensors, all before 'no CPU path'"""
    depth = torch.zeros(2, 4, 5)
    for call in (lambda d, **kw: DC.enqueue(d, None, None, 0, DC.check_params(), **kw), lambda d, **kw: DC.check_async(d, None, None, **kw)):
        refused(DC.DepthConsError, 'depth: expected torch.float32, got torch.float64', call, depth.double())
        refused(DC.DepthConsError, 'depth: expected [F, H, W], got (4, 5)', call, depth[0])
        refused(DC.DepthConsError, 'depth: expected [F, H, W], got (1, 2, 4, 5)', call, depth[None])
        refused(DC.DepthConsError, 'depth: expected a contiguous tensor, got strides (40, 10, 2) for shape (2, 4, 5)', call,
                torch.zeros(2, 4, 10)[:, :, ::2])
        refused(DC.DepthConsError, DC_NO_CPU % 'depth_out', call, depth, depth_out=np.zeros((2, 4, 5), np.float32))
        refused(DC.DepthConsError, 'depth_out: expected torch.float32, got torch.int32', call, depth, depth_out=depth.int())
        refused(DC.DepthConsError, 'depth_out: expected [F, H, W], got (4, 5)', call, depth, depth_out=depth[0].clone())
        refused(DC.DepthConsError, 'depth_out: expected a contiguous tensor, got strides (40, 10, 2) for shape (2, 4, 5)', call, depth,
                depth_out=torch.zeros(2, 4, 10)[:, :, ::2])
        refused(DC.DepthConsError, 'depth_out (2, 4, 6) on cpu: expected the shape (2, 4, 5) and device cpu of depth', call, depth,
                depth_out=torch.zeros(2, 4, 6))
        refused(DC.DepthConsError, 'depth_out (2, 4, 5) on meta: expected the shape (2, 4, 5) and device cpu of depth', call, depth,
                depth_out=torch.zeros(2, 4, 5, device='meta'))
        overlap = 'depth_out overlaps depth: the neighbours of a pixel read depth, so the check cannot run in place'
        refused(DC.DepthConsError, overlap, call, depth, depth_out=depth)
        buf = torch.zeros(3, 4, 5)
        refused(DC.DepthConsError, overlap, call, buf[:2], depth_out=buf[1:])
        refused(DC.DepthConsError, DC_NO_CPU % 'depth', call, buf[:1], depth_out=buf[1:2])       # disjoint halves of one buffer: no overlap


SIZES_REFUSED = [
    (IM, (1, 6, 6), L.NerfppError, 'nerfpp_image_metrics_workspace_bytes: a 6 x 6 image is smaller than the 7 x 7 SSIM window (H >= 7 and W >= 7)'),
    (IM, (0, 7, 7), L.NerfppError, 'nerfpp_image_metrics_workspace_bytes: n_frames = 0, expected 1 .. 65535'),
    (LP, (1, 15, 16), LP.LpipsError, 'lpips_workspace_bytes: a 15 x 16 image is too small for the four 2 x 2 pools of VGG-16 (H >= 16 and W >= 16)'),
    (LP, (0, 16, 16), LP.LpipsError, 'lpips_workspace_bytes: n_pairs = 0, expected 1 .. 65535'),
    (CC, (1, 0, 4), CC.ColorCorrectError, 'colorcc_workspace_bytes: a 0 x 4 image has no pixel (H * W >= 1)'),
    (CC, (0, 16, 16), CC.ColorCorrectError, 'colorcc_workspace_bytes: n_frames = 0, expected 1 .. 65535'),
    (DV, (1, 0), DV.DepthVisError, 'depthvis_workspace_bytes: n = 0: a frame has at least one value'),
    (DV, (0, 16), DV.DepthVisError, 'depthvis_workspace_bytes: n_frames = 0, expected 1 .. 65535'),
    (DM, (1, 0), DM.DepthMetricsError, 'depthmetrics_workspace_bytes: n_pixels = 0: a frame has at least one pixel'),
    (DM, (0, 16), DM.DepthMetricsError, 'depthmetrics_workspace_bytes: n_frames = 0, expected 1 .. 65535'),
    (DC, (1, 0, 1), DC.DepthConsError, 'depthcons_workspace_bytes: height = 0, width = 1: a frame has at least one pixel'),
    (DC, (0, 1, 1), DC.DepthConsError, 'depthcons_workspace_bytes: n_frames = 0, expected 1 .. 65535'),
]


@pytest.mark.parametrize('module,sizes,error,message', SIZES_REFUSED, ids=['%s%s' % (c[0].__name__.split('.')[-1], list(c[1])) for c in SIZES_REFUSED])
def test_negative_size_query_raises_the_librarys_words(module, sizes, error, message):
    refused(error, message, module.workspace_bytes, *sizes)
    assert module.workspace_bytes(*[max(16, s) for s in sizes]) > 0                # and the next query is answered


# ---------------------------------------------------------------------------------------------------------- Pending
class StandIn(object):
    """what Pending asks of a device tensor: .cpu().numpy(), counted"""

    def __init__(self, values):
        self.values, self.reads = np.asarray(values), 0

    def cpu(self):
        self.reads += 1
        return self

    def numpy(self):
        return self.values


class Kept(object):
    pass


def test_pending_reads_once_and_lets_go():
    a, b, kept = StandIn([1., 2.]), StandIn([[3]]), Kept()
    alive = weakref.ref(kept)
    pend = U.Pending({'a': a, 'b': b}, (kept, 'x'))
    del kept
    assert pend.tensors == {'a': a, 'b': b} and (a.reads, b.reads) == (0, 0) and alive() is not None
    host = pend.get()
    assert set(host) == {'a', 'b'} and host['a'] is a.values and host['b'] is b.values
    assert alive() is None                                # keep is released by the first read
    assert pend.get() is host and (a.reads, b.reads) == (1, 1) and pend.tensors == {'a': a, 'b': b}


def test_pending_applies_its_host_function_once():
    a, calls = StandIn([1., 2.]), []

    def to_host(tensors):
        calls.append(tensors)
        return tensors['a'].cpu().numpy() * 2, None

    pend = U.Pending({'a': a}, None, to_host)
    assert not calls
    host = pend.get()
    assert pend.get() is host and len(calls) == 1 and calls[0] is pend.tensors and a.reads == 1
    assert list(host[0]) == [2., 4.] and host[1] is None


# ------------------------------------------------------------------------------------------------------------- GPU
def _dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _rand(shape, dtype, dev, seed=0):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, shape).astype(np.uint8) if dtype == torch.uint8 else rs.uniform(0.05, 1.0, shape)
    return torch.from_numpy(a).to(device=dev, dtype=dtype)


def _both_u8(call, error):
    dev = _dev()
    u8, f32 = _rand((2, 16, 16, 3), torch.uint8, dev), _rand((2, 16, 16, 3), torch.float32, dev)
    refused(error, 'gt_u8: expected uint8 (the bytes written to the PNG), got torch.float32', call, f32, u8)
    refused(error, 'pred_u8: expected uint8 (the bytes written to the PNG), got torch.float32', call, u8, f32)
    refused(error, 'gt_u8: expected [H, W, 3] or [F, H, W, 3], got (1, 16, 16, 4)', call, _rand((16, 16, 4), torch.uint8, dev), u8)
    refused(error, 'pred_u8: expected [H, W, 3] or [F, H, W, 3], got (16, 3)', call, u8, u8[0, 0])
    refused(error, 'pred_u8: expected [H, W, 3] or [F, H, W, 3], got (1, 2, 16, 16, 3)', call, u8, u8[None])
    refused(error, 'gt_u8 (2, 16, 16, 3) and pred_u8 (1, 16, 16, 3) differ in shape', call, u8, u8[0])


@gpu
def test_image_metrics_refusals_on_device_tensors():
    _both_u8(IM.image_metrics_async, L.NerfppError)


@gpu
def test_lpips_refusals_on_device_tensors():
    _both_u8(lambda g, p: LP.lpips_u8(g, p, _weights()), LP.LpipsError)


@gpu
@pytest.mark.parametrize('call', [CC.color_correct_async, CC.normal_equations], ids=['color_correct_async', 'normal_equations'])
def test_color_correct_refusals_on_device_tensors(call):
    dev, E = _dev(), CC.ColorCorrectError
    img, ref = _rand((2, 16, 16, 3), torch.float32, dev), _rand((2, 16, 16, 3), torch.uint8, dev)
    refused(E, 'img_f32: expected torch.float32, got torch.uint8', call, ref, ref)
    refused(E, 'ref_u8: expected torch.uint8, got torch.float32', call, img, img)
    refused(E, 'ref_u8: expected a CUDA/HIP torch.uint8 tensor (color_correct has no CPU path)', call, img, ref.cpu())
    refused(E, 'img_f32: expected [H, W, 3] or [F, H, W, 3], got (2, 16, 16, 2)', call, img[..., :2], ref)
    refused(E, 'img_f32: expected [H, W, 3] or [F, H, W, 3], got (16, 3)', call, img[0, 0], ref)
    refused(E, 'img_f32 (2, 16, 16, 3) and ref_u8 (1, 16, 16, 3) differ in shape', call, img, ref[0])
    refused(E, 'img_f32 (2, 16, 16, 3) and ref_u8 (2, 16, 16, 4) differ in shape', call, img, _rand((2, 16, 16, 4), torch.uint8, dev))


@gpu
def test_depth_metrics_refusals_on_device_tensors():
    dev, E = _dev(), DM.DepthMetricsError
    pred, gt = _rand((2, 16, 8), torch.float32, dev), _rand((2, 16, 16), torch.float32, dev, 1)
    call = lambda p, g: DM.depth_metrics_async(p, g, 1.0)
    refused(E, 'pred: expected torch.float32, got torch.float64', call, pred.double(), pred)
    refused(E, 'gt: expected torch.float32, got torch.float16', call, pred, pred.half())
    refused(E, 'gt: expected a CUDA/HIP float32 tensor (the depth metrics have no CPU path)', call, pred, pred.cpu())
    refused(E, 'pred: expected [F, H, W] or [H, W], got (2, 16, 16, 3)', call, _rand((2, 16, 16, 3), torch.float32, dev), pred)
    refused(E, 'gt: expected [F, H, W] or [H, W], got (8,)', call, pred, pred[0, 0])
    refused(E, 'gt: expected a contiguous tensor, got strides (256, 16, 2) for shape (2, 16, 8)', call, pred, gt[:, :, ::2])
    refused(E, 'pred: expected a contiguous tensor, got strides (256, 16, 2) for shape (1, 16, 8)', call, gt[0, :, ::2], pred[0])   # the batch axis first
    refused(E, 'pred (2, 16, 8) and gt (1, 16, 8): shapes differ', call, pred, pred[0])


@gpu
def test_depth_vis_refusals_on_device_tensors():
    dev, E = _dev(), DV.DepthVisError
    v, rgb = _rand((2, 16, 16), torch.float32, dev), _rand((2, 16, 16, 3), torch.float32, dev, 1)
    refused(E, 'value: expected torch.float32, got torch.float64', DV.minmax_colorize_async, v.double())
    refused(E, 'weight: expected torch.float32, got torch.float64', DV.weighted_percentiles_async, v[0], v[0].double(), (50.,))
    refused(E, 'acc: expected a CUDA/HIP float32 tensor (the depth pictures have no CPU path)', DV.matte_rgb_async, rgb, v.cpu())
    refused(E, 'rgb: shape (2, 16, 16, 2) does not end in (3,)', DV.matte_rgb_async, rgb[..., :2], v)
    refused(E, 'value: shape (2, 16, 16) does not end in (3,)', DV.colorize_cmap_async, v, v, cmap=None)
    refused(E, 'rgb: expected [F, H, W, 3], got (3,)', DV.matte_rgb_async, rgb[0, 0, 0], v)
    refused(E, 'value: expected [F, H, W], got (16,)', DV.minmax_colorize_async, v[0, 0])
    refused(E, 'value: expected [F, H, W], got (2, 16, 16, 3)', DV.minmax_colorize_async, rgb)
    refused(E, 'value (2, 16) and weight (2, 8): expected two [F, N] tensors on one device', DV.weighted_percentiles_async,
            v[:, 0], v[:, 0, :8], (50.,))
    refused(E, 'value (2, 16, 16) and weight (2, 16, 16): expected two [F, N] tensors on one device', DV.weighted_percentiles_async, v, v, (50.,))
    refused(E, 'ps: 5 percentiles, expected 1 .. 4', DV.weighted_percentiles_async, v[0], v[0], (1., 2., 3., 4., 5.))
    refused(E, 'value (2, 16, 16) and acc (1, 16, 16) differ in frame shape or device', DV.colorize_cmap_async, v, v[0])
    refused(E, 'colorize_cmap_async: a 3-channel value needs lohi (mip360_suite_async computes it)', DV.colorize_cmap_async, rgb, v, cmap=None)
    refused(E, 'rgb (2, 16, 16, 3) and acc (1, 16, 16) differ in frame shape', DV.matte_rgb_async, rgb, v[0])
    refused(E, 'directions (1, 16, 16, 3) and acc (2, 16, 16) differ in frame shape', DV.coords_mod_async, rgb, rgb[0], v, v)
    refused(E, 'mip360_suite_async: inputs differ in frame shape (2, 16, 16) or device', DV.mip360_suite_async, rgb, v, v, v[0], v, v, rgb, rgb)
    refused(E, 'mip360_depth_pair_async: inputs differ in frame shape', DV.mip360_depth_pair_async, v, v[0], v)


@gpu
def test_depth_consistency_refusals_on_device_tensors():
    dev, E = _dev(), DC.DepthConsError
    depth = _rand((2, 16, 16), torch.float32, dev)
    prm = DC.check_params()
    refused(E, 'depth_out (2, 16, 16) on cpu: expected the shape (2, 16, 16) and device cuda:0 of depth', DC.enqueue, depth, None, None, 0, prm,
            depth_out=depth.cpu())
    refused(E, 'depth_out overlaps depth: the neighbours of a pixel read depth, so the check cannot run in place', DC.enqueue, depth, None, None,
            0, prm, depth_out=depth)
    refused(E, 'cams: 3 cameras for 2 frames of depth', DC.enqueue, depth, torch.zeros(3, DC.CAM, dtype=torch.float64, device=dev), None, 0, prm)


@gpu
def test_a_pair_on_two_devices_is_refused():
    dev = _dev()
    if torch.cuda.device_count() < 2:
        pytest.skip('needs 2 GPUs, found %d' % torch.cuda.device_count())
    u8, f32 = _rand((2, 16, 16, 3), torch.uint8, dev), _rand((2, 16, 16, 3), torch.float32, dev)
    v = f32[..., 0].contiguous()
    refused(L.NerfppError, 'gt_u8 and pred_u8 live on different devices', IM.image_metrics_async, u8, u8.to('cuda:1'))
    refused(LP.LpipsError, 'gt_u8 and pred_u8 live on different devices', LP.lpips_u8, u8, u8.to('cuda:1'), _weights())
    for call in (CC.color_correct_async, CC.normal_equations):
        refused(CC.ColorCorrectError, 'img_f32 and ref_u8 live on different devices', call, f32, u8.to('cuda:1'))
    refused(DM.DepthMetricsError, 'pred on cuda:0 and gt on cuda:1: devices differ', DM.depth_metrics_async, v, v.to('cuda:1'), 1.0)
    refused(DV.DepthVisError, 'value (2, 16, 16) and acc (2, 16, 16) differ in frame shape or device', DV.colorize_cmap_async, v, v.to('cuda:1'))
    refused(DV.DepthVisError, 'value (2, 16) and weight (2, 16): expected two [F, N] tensors on one device', DV.weighted_percentiles_async,
            v[:, 0], v[:, 0].to('cuda:1'), (50.,))
    refused(DV.DepthVisError, 'mip360_suite_async: inputs differ in frame shape (2, 16, 16) or device', DV.mip360_suite_async,
            f32, v, v, v.to('cuda:1'), v, v, f32, f32)
    refused(DC.DepthConsError, 'depth_out (2, 16, 16) on cuda:1: expected the shape (2, 16, 16) and device cuda:0 of depth', DC.enqueue,
            v, None, None, 0, DC.check_params(), depth_out=v.to('cuda:1'))


# --- the workspace cache
def _depth_pair(n, dev):
    return _rand((1, 1, n), torch.float32, dev, n) * 40, _rand((1, 1, n), torch.float32, dev, 100 + n) * 40


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


@gpu
def test_workspace_cache_holds_two_shapes_and_clears_when_full():
    """depth_metrics holds two shapes: frames of 1 x 2, 1 x 3, 1 x 4 pixels -- the third clears the cache, the first then gets a fresh
    buffer, and the result that was pending on the evicted buffer is still right (it kept the buffer)"""
    dev = _dev()
    cache, i = DM._workspaces, dev.index
    cache.clear()
    first = DM.depth_metrics_async(*_depth_pair(2, dev), 1.0, err_map=True)
    ws = cache.buffer(dev, 1, 2)
    assert list(cache) == [(i, 1, 2)] and cache.buffer(dev, 1, 2) is ws and cache[(i, 1, 2)] is ws
    assert ws.dtype == torch.float64 and ws.numel() == DM.workspace_bytes(1, 2) // 8 and ws.device == dev
    DM.depth_metrics_async(*_depth_pair(3, dev), 1.0)
    assert list(cache) == [(i, 1, 2), (i, 1, 3)] and cache.buffer(dev, 1, 2) is ws
    DM.depth_metrics_async(*_depth_pair(4, dev), 1.0)
    assert list(cache) == [(i, 1, 4)]
    alive = weakref.ref(ws)
    fresh = cache.buffer(dev, 1, 2)
    assert fresh is not ws and list(cache) == [(i, 1, 4), (i, 1, 2)]
    del ws
    assert alive() is not None                            # evicted, but the pending result holds it until it is read
    want = DM.depth_metrics(*_depth_pair(2, dev), 1.0, err_map=True)
    np.testing.assert_array_equal(first.tensors['rows'].cpu().numpy(), np.stack([want[k] for k in DM.METRIC_NAMES], 1))
    np.testing.assert_array_equal(first.tensors['err_map'].cpu().numpy(), want['err_map'])
    _same(first.get(), want)
    assert alive() is None and first.get() is first.get()


@gpu
def test_workspace_cache_of_one_shape_evicts_on_the_next():
    """color_correct holds one shape: frames of 1 x 1, then 1 x 2"""
    dev = _dev()
    cache, i = CC._workspaces, dev.index
    cache.clear()
    img, ref = _rand((1, 1, 1, 3), torch.float32, dev), _rand((1, 1, 1, 3), torch.uint8, dev, 1)
    first = CC.color_correct_async(img, ref)
    alive = weakref.ref(cache[(i, 1, 1, 1)])
    assert list(cache) == [(i, 1, 1, 1)] and cache.buffer(dev, 1, 1, 1) is alive()
    assert alive().dtype == torch.float64 and alive().numel() == CC.workspace_bytes(1, 1, 1) // 8
    CC.color_correct_async(_rand((1, 1, 2, 3), torch.float32, dev), _rand((1, 1, 2, 3), torch.uint8, dev, 1))
    assert list(cache) == [(i, 1, 1, 2)] and alive() is not None
    want = CC.color_correct(img, ref)
    assert list(cache) == [(i, 1, 1, 1)] and cache[(i, 1, 1, 1)] is not alive()
    np.testing.assert_array_equal(first.tensors['rgb_cc'].cpu().numpy(), want[0])
    np.testing.assert_array_equal(first.tensors['cc_u8'].cpu().numpy(), want[1])
    got = first.get()
    assert alive() is None and first.get() is got and len(got) == 4
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


@gpu
def test_consistency_workspace_is_int32_and_only_for_rows():
    dev = _dev()
    cache = DC._workspaces
    cache.clear()
    depth = _rand((2, 16, 16), torch.float32, dev) + 1
    cams = np.tile(np.array([[20., 20., 8., 8., 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]]), (2, 1))
    cams[1, 7] = 0.1
    DC.check_async(depth, cams, DC.neighbours(cams[:, [7, 11, 15]], 1), rows=False).get()
    assert list(cache) == []
    got = DC.check_async(depth, cams, DC.neighbours(cams[:, [7, 11, 15]], 1)).get()
    ws = cache[(dev.index, 2, 16, 16)]
    assert ws.dtype == torch.int32 and ws.numel() == DC.workspace_bytes(2, 16, 16) // 4 and got['rows'].shape == (2, 4)


# --- non-contiguous inputs where the binding copies
def _every_other(shape, dtype, dev, seed=0):
    """(a non-contiguous view of `shape`, its contiguous copy)"""
    wide = _rand(shape[:2] + (2 * shape[2],) + shape[3:], dtype, dev, seed)
    view = wide[:, :, ::2]
    assert not view.is_contiguous() and tuple(view.shape) == shape
    return view, view.contiguous()


def _same_tuple(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@gpu
def test_image_metrics_and_lpips_copy_non_contiguous_frames():
    from tests.test_gpu_lpips import weights
    dev = _dev()
    (g, gc), (p, pc) = _every_other((2, 16, 16, 3), torch.uint8, dev), _every_other((2, 16, 16, 3), torch.uint8, dev, 1)
    _same_tuple(IM.image_metrics(g, p), IM.image_metrics(gc, pc))
    _same_tuple(LP.lpips_u8(g, p, weights()[1]), LP.lpips_u8(gc, pc, weights()[1]))


@gpu
def test_color_correct_copies_non_contiguous_frames():
    dev = _dev()
    (img, imgc), (ref, refc) = _every_other((2, 16, 16, 3), torch.float32, dev), _every_other((2, 16, 16, 3), torch.uint8, dev, 1)
    _same_tuple(CC.color_correct(img, ref), CC.color_correct(imgc, refc))
    np.testing.assert_array_equal(CC.normal_equations(img, ref), CC.normal_equations(imgc, refc))


@gpu
def test_depth_vis_copies_non_contiguous_frames():
    dev = _dev()
    (v, vc), (a, ac) = _every_other((2, 16, 16), torch.float32, dev), _every_other((2, 16, 16), torch.float32, dev, 1)
    (rgb, rgbc), (o, oc) = _every_other((2, 16, 16, 3), torch.float32, dev, 2), _every_other((2, 16, 16, 3), torch.float32, dev, 3)
    _same(DV.minmax_colorize_async(v).get(), DV.minmax_colorize_async(vc).get())
    _same(DV.colorize_cmap_async(v, a).get(), DV.colorize_cmap_async(vc, ac).get())
    _same(DV.matte_rgb_async(rgb, a).get(), DV.matte_rgb_async(rgbc, ac).get())
    _same(DV.coords_mod_async(o, rgb, v, a).get(), DV.coords_mod_async(oc, rgbc, vc, ac).get())
    _same(DV.mip360_depth_pair_async(v, v, a).get(), DV.mip360_depth_pair_async(vc, vc, ac).get())
    _same(DV.mip360_suite_async(rgb, a, v, v, v, v, o, rgb).get(), DV.mip360_suite_async(rgbc, ac, vc, vc, vc, vc, oc, rgbc).get())
    np.testing.assert_array_equal(DV.weighted_percentiles(v.reshape(2, -1)[:, ::2], a.reshape(2, -1)[:, ::2], (5., 50.)),
                                  DV.weighted_percentiles(vc.reshape(2, -1)[:, ::2].contiguous(), ac.reshape(2, -1)[:, ::2].contiguous(), (5., 50.)))
    np.testing.assert_array_equal(DV.minmax(v), DV.minmax(vc))
