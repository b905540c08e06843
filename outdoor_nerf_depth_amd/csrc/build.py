"""Build libnerfpp_hip.so, libmip360_hip.so, liblpips_hip.so, libcolorcc_hip.so, libdepthvis_hip.so, libdepthmetrics_hip.so, libdepthssi_hip.so, libdepthgnll_hip.so, libdepthcons_hip.so, libdepthacc_hip.so, libdepthalign_hip.so, libdepthcomp_hip.so, libdepthmvs_hip.so, libdepthsgm_hip.so, libdepthpoints_hip.so, librayreg_hip.so, libdepthguide_hip.so and libraylos_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python outdoor_nerf_depth_amd/csrc/build.py [--force]
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
OBJ = os.path.join(HERE, 'build')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
COMMON = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function',
          '-fhip-fp32-correctly-rounded-divide-sqrt']
INCLUDE = os.path.join('..', '..', 'include')
# One entry per shared object: (file name in the package, {source: extra flags}, headers every source of it depends on).
# A source given as (file, k) is one translation unit per k: object <file>_<k>.o.
# headers of every library: device vocabulary, C-ABI preamble, what the depth-prior libraries share on the device
SHARED = ['hip_device.h', 'api_common.h', 'depth_prior_device.h']
LIBRARIES = [
    ('libnerfpp_hip.so', {
        'nerfpp_tables.hip': [],
        'nerfpp_render.hip': ['-ffp-contract=off'],     # bit-exact sample bins: no implicit FMA
        # the fully unrolled MLP kernels: one translation unit per instantiation (nerfpp_mlp.hip, NERFPP_MLP_PART)
        **{('nerfpp_mlp.hip', k): ['-DNERFPP_MLP_PART=%d' % k] for k in range(9)},
        'nerfpp_dw.hip': [],
        'nerfpp_optim.hip': ['-ffp-contract=off'],      # Adam rounds like torch
        'nerfpp_api.hip': [],
        'image_metrics.hip': ['-ffp-contract=off'],     # SSIM in float64 in scikit-image's written order: no implicit FMA
        'nerfpp_comm.hip': [],                         # RCCL entry points (librccl.so.1 bound with dlopen at first use)
    }, ['nerfpp_common.h', 'nerfpp_kernels.h', 'probe_env.h', 'nerfpp_mlp_probes.h', 'nerfpp_mlp_split.h',
        os.path.join(INCLUDE, 'nerfpp_hip.h')] + SHARED),
    # SURVEY 8 f-4 (MipNeRF-360 path): its own shared object and C ABI (include/mip360_hip.h)
    ('libmip360_hip.so', {
        'mip360_kernels.hip': ['-ffp-contract=off'],    # arithmetic order of the oracle
        'mip360_gemm.hip': [],
        'mip360_fm.hip': [],
        'mip360_prop.hip': [],                          # the PropMLP forward / dX chain as one launch each
        'mip360_view.hip': [],                          # the NerfMLP's view branch forward as one launch
        'mip360_train.hip': [],
        'mip360_glo.hip': ['-ffp-contract=off'],       # per-image embeddings: mip360_dir_encode's bytes in the table
        'mip360_rays.hip': ['-ffp-contract=off'],      # camera rays, training batch, distance percentiles: the written order
        'mip360_depth_rays.hip': ['-ffp-contract=off'],  # per-ray kl / urf depth losses: float32 near / empty as written
        'mip360_api.hip': [],
    }, ['mip360_device.h', 'mip360_launch.h', 'probe_env.h', 'mip360_gemm_probes.h', 'mip360_fm_probes.h',
        os.path.join(INCLUDE, 'mip360_hip.h')] + SHARED),
    # LPIPS from user-supplied weights: its own shared object and C ABI (include/lpips_hip.h)
    ('liblpips_hip.so', {
        'lpips_conv.hip': [],                           # float32 MFMA implicit GEMM
        'lpips_tap.hip': ['-ffp-contract=off'],         # input scaling and tap sums in the written order
        'lpips_api.hip': [],
    }, ['lpips_kernels.h', os.path.join(INCLUDE, 'lpips_hip.h')] + SHARED),
    # colour-corrected test renders: its own shared object and C ABI (include/colorcc_hip.h)
    ('libcolorcc_hip.so', {
        'colorcc_kernels.hip': ['-ffp-contract=off'],   # accumulate and apply rebuild a pixel with the same bits: explicit fma only
        'colorcc_api.hip': [],
    }, ['colorcc_kernels.h', os.path.join(INCLUDE, 'colorcc_hip.h')] + SHARED),
    # depth pictures of the evaluators: its own shared object and C ABI (include/depthvis_hip.h)
    ('libdepthvis_hip.so', {
        'depthvis_kernels.hip': ['-ffp-contract=off'],  # float64 in the written order: the bytes of the numpy restatement
        'depthvis_api.hip': [],
    }, ['depthvis_kernels.h', os.path.join(INCLUDE, 'depthvis_hip.h')] + SHARED),
    # depth-error metrics of the evaluators: its own shared object and C ABI (include/depthmetrics_hip.h)
    ('libdepthmetrics_hip.so', {
        'depthmetrics_kernels.hip': ['-ffp-contract=off'],  # float64 sums of the written terms: no implicit FMA
        'depthmetrics_api.hip': [],
    }, ['depthmetrics_kernels.h', os.path.join(INCLUDE, 'depthmetrics_hip.h')] + SHARED),
    # scale-and-shift-invariant depth loss of both training paths: its own shared object and C ABI (include/depthssi_hip.h)
    ('libdepthssi_hip.so', {
        'depthssi_kernels.hip': ['-ffp-contract=off'],  # float64 sums, solve and residuals as written: no implicit FMA
        'depthssi_api.hip': [],
    }, ['depthssi_kernels.h', os.path.join(INCLUDE, 'depthssi_hip.h')] + SHARED),
    # Gaussian-NLL depth loss for priors with a standard deviation, both training paths: its own shared object and C ABI
    # (include/depthgnll_hip.h)
    ('libdepthgnll_hip.so', {
        'depthgnll_kernels.hip': ['-ffp-contract=off'],  # float64 sums, gate and gradients as written: no implicit FMA
        'depthgnll_api.hip': [],
    }, ['depthgnll_kernels.h', os.path.join(INCLUDE, 'depthgnll_hip.h')] + SHARED),
    # multi-view consistency check of depth priors: its own shared object and C ABI (include/depthcons_hip.h)
    ('libdepthcons_hip.so', {
        'depthcons_kernels.hip': ['-ffp-contract=off'],  # float64 geometry in the written order: the decisions of the numpy restatement
        'depthcons_api.hip': [],
    }, ['depthcons_kernels.h', os.path.join(INCLUDE, 'depthcons_hip.h')] + SHARED),
    # densifying sparse depth priors from neighbouring frames: its own shared object and C ABI (include/depthacc_hip.h)
    ('libdepthacc_hip.so', {
        'depthacc_kernels.hip': ['-ffp-contract=off'],  # float64 geometry in the written order: the keys of the numpy restatement
        'depthacc_api.hip': [],
    }, ['depthacc_kernels.h', os.path.join(INCLUDE, 'depthacc_hip.h')] + SHARED),
    # aligning relative depth priors to sparse metric depth: its own shared object and C ABI (include/depthalign_hip.h)
    ('libdepthalign_hip.so', {
        'depthalign_kernels.hip': ['-ffp-contract=off'],  # float64 sums, solves and the apply step as written: no implicit FMA
        'depthalign_api.hip': [],
    }, ['depthalign_kernels.h', os.path.join(INCLUDE, 'depthalign_hip.h')] + SHARED),
    # completing sparse depth priors by image-guided filtering: its own shared object and C ABI (include/depthcomp_hip.h)
    ('libdepthcomp_hip.so', {
        'depthcomp_kernels.hip': ['-ffp-contract=off'],  # float64 window sums in the written order: the bits of the numpy restatement
        'depthcomp_api.hip': [],
    }, ['depthcomp_kernels.h', os.path.join(INCLUDE, 'depthcomp_hip.h')] + SHARED),
    # plane-sweep multi-view stereo depth prior: its own shared object and C ABI (include/depthmvs_hip.h)
    ('libdepthmvs_hip.so', {
        'depthmvs_kernels.hip': ['-ffp-contract=off'],  # float64 geometry and refinement in the written order: the bits of the numpy restatement
        'depthmvs_api.hip': [],
    }, ['depthmvs_kernels.h', 'depthmvs_sweep.h', os.path.join(INCLUDE, 'depthmvs_hip.h')] + SHARED),
    # the plane sweep with semi-global smoothing: its own shared object and C ABI (include/depthsgm_hip.h); the sweep's
    # kernels come from the one definition in depthmvs_sweep.h
    ('libdepthsgm_hip.so', {
        'depthsgm_kernels.hip': ['-ffp-contract=off'],  # the sweep's float64 geometry and refinement in the written order
        'depthsgm_api.hip': [],
    }, ['depthsgm_kernels.h', 'depthmvs_kernels.h', 'depthmvs_sweep.h', os.path.join(INCLUDE, 'depthsgm_hip.h'),
        os.path.join(INCLUDE, 'depthmvs_hip.h')] + SHARED),
    # sparse depth prior from the reconstruction's point cloud: its own shared object and C ABI (include/depthpoints_hip.h)
    ('libdepthpoints_hip.so', {
        'depthpoints_kernels.hip': ['-ffp-contract=off'],  # float64 geometry in the written order: the keys of the numpy restatement
        'depthpoints_api.hip': [],
    }, ['depthpoints_kernels.h', os.path.join(INCLUDE, 'depthpoints_hip.h')] + SHARED),
    # distortion and opacity regularisers on the foreground weights of the NeRF++ path: its own shared object and C ABI
    # (include/rayreg_hip.h)
    ('librayreg_hip.so', {
        'rayreg_kernels.hip': ['-ffp-contract=off'],  # float64 prefix sums and gradients as written: no implicit FMA
        'rayreg_api.hip': [],
    }, ['rayreg_kernels.h', os.path.join(INCLUDE, 'rayreg_hip.h')] + SHARED),
    # depth-guided fine sampling of the NeRF++ path: its own shared object and C ABI (include/depthguide_hip.h); the
    # Philox generator comes from the one definition in nerfpp_common.h
    ('libdepthguide_hip.so', {
        'depthguide_kernels.hip': ['-ffp-contract=off'],  # float64 moments and positions as written: the bits of the numpy restatement
        'depthguide_api.hip': [],
    }, ['depthguide_kernels.h', 'nerfpp_common.h', os.path.join(INCLUDE, 'depthguide_hip.h')] + SHARED),
    # Urban Radiance Fields' line-of-sight term on the foreground weights of the NeRF++ path: its own shared object and
    # C ABI (include/raylos_hip.h)
    ('libraylos_hip.so', {
        'raylos_kernels.hip': ['-ffp-contract=off'],  # float32 band bounds and comparisons as written: no implicit FMA
        'raylos_api.hip': [],
    }, ['raylos_kernels.h', os.path.join(INCLUDE, 'raylos_hip.h')] + SHARED),
]
OUT = os.path.join(PKG, LIBRARIES[0][0])


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def split_source(src):
    """'a.hip' or ('a.hip', k) -> (file name, object name)"""
    if isinstance(src, tuple):
        return src[0], src[0].replace('.hip', '_%d.o' % src[1])
    return src, src.replace('.hip', '.o')


def _compile(src, flags, headers):
    src, obj = split_source(src)
    obj = os.path.join(OBJ, obj)
    deps = [os.path.join(HERE, src)] + [os.path.join(HERE, h) for h in headers] + [__file__]
    if _stale(obj, deps):
        subprocess.check_call([HIPCC] + COMMON + flags + ['-c', os.path.join(HERE, src), '-o', obj])
    return obj


def build(force=False):
    os.makedirs(OBJ, exist_ok=True)
    if force:
        for f in os.listdir(OBJ):
            if os.path.isfile(os.path.join(OBJ, f)):
                os.remove(os.path.join(OBJ, f))
    with ThreadPoolExecutor(max_workers=int(os.environ.get('NERFPP_BUILD_JOBS', '8'))) as ex:
        jobs = [[ex.submit(_compile, src, flags, headers) for src, flags in sources.items()] for _, sources, headers in LIBRARIES]
        for (name, _, _), lib_jobs in zip(LIBRARIES, jobs):
            objs = [j.result() for j in lib_jobs]
            out = os.path.join(PKG, name)
            if force or _stale(out, objs):
                subprocess.check_call([HIPCC, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', out] + objs)
    return OUT


if __name__ == '__main__':
    print(build(force='--force' in sys.argv))
