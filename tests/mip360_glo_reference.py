"""float64 restatement (torch CPU, autograd) of the NerfMLP's view branch with per-image appearance embeddings (GLO):
internal/models.py:560-606 with glo_vec -- x = [bottleneck, pos_enc(viewdirs, 0, 4, append_identity), embed[cam]] ->
Dense(128) + ReLU -> Dense(3) -> sigmoid * (1 + 2 rgb_padding) - rgb_padding -- and the bottleneck head in front of it.
Kernels are in flax layout [in, out].  The direction encoding is oracle/mip360_oracle.py's.

round_like_kernels=True rounds to bfloat16 at the points where the HIP path rounds a GEMM operand (the restatement
tests/test_gpu_mip360.py::_mlp_bf16_fwd_bwd makes by hand, here through autograd): forward the bottleneck and the hidden layer,
backward d rgb_pre, d_hz (the hidden layer's pre-activation cotangent) and d_bott.  Everything else stays float64."""
import numpy as np
import torch

from oracle import mip360_oracle as O

RGB_PADDING = 0.001
BOTTLENECK, DIR_DIM = 256, 27


def t64(a):
    return a.double() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, np.float64))


def _round_bf16(t):
    return t.detach().float().bfloat16().double()


class _RoundForward(torch.autograd.Function):
    """bfloat16 rounding of a value; the cotangent passes unchanged (the kernels' stored operand is the rounded one)"""
    @staticmethod
    def forward(ctx, x):
        return _round_bf16(x)

    @staticmethod
    def backward(ctx, g):
        return g


def _round_cotangent(t):
    if t.requires_grad:
        t.register_hook(_round_bf16)
    return t


def dir_features(viewdirs):
    """pos_enc(viewdirs, min_deg 0, max_deg 4, append_identity=True) -> [n, 27]"""
    return t64(O.pos_enc(np.asarray(viewdirs, np.float64), 0, 4, True))


def view_input(bott, dir_feat, embed=None, cam=None):
    """[bottleneck | direction features | embed[cam]] per row (upstream's order); embed None = no GLO columns"""
    parts = [t64(bott), t64(dir_feat)]
    if embed is not None and embed.shape[1] > 0:
        parts.append(embed[torch.as_tensor(np.asarray(cam), dtype=torch.long)])
    return torch.cat(parts, -1)


def view_branch(x, w1, b1, w2, b2, round_like_kernels=False):
    """(rgb [rows, 3], h [rows, 128]) of the two dense layers and the padded sigmoid"""
    pre = x @ t64(w1) + t64(b1)
    if round_like_kernels:
        pre = _round_cotangent(pre)                              # d_hz is stored as bf16
    h = torch.relu(pre)
    if round_like_kernels:
        h = _RoundForward.apply(h)
    raw = h @ t64(w2) + t64(b2)
    if round_like_kernels:
        raw = _round_cotangent(raw)                              # d rgb_pre is stored as bf16
    return torch.sigmoid(raw) * (1 + 2 * RGB_PADDING) - RGB_PADDING, h


def trunk_head(x_trunk, w_bott, b_bott, round_like_kernels=False):
    """the bottleneck Dense(256) on the trunk's last activation (models.py:560-563)"""
    bott = t64(x_trunk) @ t64(w_bott) + t64(b_bott)
    if round_like_kernels:
        bott = _RoundForward.apply(_round_cotangent(bott))      # the bottleneck and d_bott are stored as bf16
    return bott


def embed_grad_from_dhz(d_hz, w_view, cam, n_samples, n_embed, n_features):
    """sum over a camera's rays and their samples of d_hz . W_view[283 + g]: [n_embed, n_features] float64, and the sum of
    |products| per entry (the scale of the float32 accumulation error)"""
    d = np.asarray(d_hz, np.float64)
    w = np.asarray(w_view, np.float64)[BOTTLENECK + DIR_DIM:BOTTLENECK + DIR_DIM + n_features]        # [G, 128]
    per_row, per_row_abs = d @ w.T, np.abs(d) @ np.abs(w).T
    cam_rows = np.repeat(np.asarray(cam, np.int64), n_samples)
    g, a = np.zeros((n_embed, n_features)), np.zeros((n_embed, n_features))
    np.add.at(g, cam_rows, per_row)
    np.add.at(a, cam_rows, per_row_abs)
    return g, a
