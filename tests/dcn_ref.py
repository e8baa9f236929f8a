"""Float64 restatement of the modulated deformable conv (DCNv2) in plain torch: the yardstick of tests/test_dcn_*.py.

Semantics (the reference's source/cpu/dcn.im2col.cpp:156-190 and dcn_v2.py:146-191, on NHWC tensors): 3x3 taps
k = 3i + j, stride 1, pad 1, dilation 1, G deformable groups of C/G channels.  For output pixel (h, w), tap k, group g:
dh = off[18g + 2k], dw = off[18g + 2k + 1], m = mask[9g + k]; the sample point is (h - 1 + i + dh, w - 1 + j + dw);
col[k][c] = m * sum over the 4 bilinear corners of weight * x[corner][c], a corner outside [0,H-1] x [0,W-1]
contributing 0; y[co] = bias[co] + sum_{k,c} weight[co][c][i][j] * col[k][c].

Two independent formulations of the columns, held to each other by tests/test_dcn_cpu.py:
  cols_gather   an index gather per corner, straight from the formula
  cols_grid     F.grid_sample(bilinear, zeros, align_corners=True) per tap and group (needs H, W > 1)
Both are differentiable by autograd in every input.  What autograd cannot give -- the sums of absolute terms the GPU
tests' bounds are stated in, and the per-element contribution counts -- is written out from the same corner walk.
"""
import torch
import torch.nn.functional as F


def corners(off, H, W, g, k):
    """The four bilinear corners of tap k, group g at every pixel: a list of (flat index into H*W (clamped), inside,
    weight, d weight / d h, d weight / d w), each (N,H,W)."""
    i, j = divmod(k, 3)
    hh = torch.arange(H, dtype=off.dtype).view(1, H, 1)
    ww = torch.arange(W, dtype=off.dtype).view(1, 1, W)
    ph = hh - 1 + i + off[..., 18 * g + 2 * k]
    pw = ww - 1 + j + off[..., 18 * g + 2 * k + 1]
    h0, w0 = torch.floor(ph).detach(), torch.floor(pw).detach()
    lh, lw = ph - h0, pw - w0
    out = []
    for a in (0, 1):
        for b in (0, 1):
            hi, wi = h0 + a, w0 + b
            ok = (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
            idx = (hi.clamp(0, H - 1) * W + wi.clamp(0, W - 1)).long()
            fh, fw = (lh if a else 1 - lh), (lw if b else 1 - lw)
            out.append((idx, ok, fh * fw, (1.0 if a else -1.0) * fw, (1.0 if b else -1.0) * fh))
    return out


def _take(xg, idx):
    """xg (N, H*W, Cg) gathered at idx (N,H,W) -> (N,H,W,Cg)."""
    N, Hh, Ww = idx.shape
    return torch.gather(xg, 1, idx.reshape(N, -1, 1).expand(-1, -1, xg.shape[2])).view(N, Hh, Ww, xg.shape[2])


def cols_gather(x, off, mask, G):
    """(N,H,W,C), (N,H,W,18G), (N,H,W,9G) -> columns (N,H,W,9,C)."""
    N, H, W, C = x.shape
    Cg = C // G
    taps = []
    for k in range(9):
        groups = []
        for g in range(G):
            xg = x[..., g * Cg:(g + 1) * Cg].reshape(N, H * W, Cg)
            val = 0
            for idx, ok, wt, _, _ in corners(off, H, W, g, k):
                val = val + (wt * ok).unsqueeze(-1) * _take(xg, idx)
            groups.append(mask[..., 9 * g + k].unsqueeze(-1) * val)
        taps.append(torch.cat(groups, -1))
    return torch.stack(taps, 3)


def cols_grid(x, off, mask, G):
    """The same columns through F.grid_sample (H, W > 1)."""
    N, H, W, C = x.shape
    Cg = C // G
    xn = x.permute(0, 3, 1, 2)
    hh = torch.arange(H, dtype=x.dtype).view(1, H, 1)
    ww = torch.arange(W, dtype=x.dtype).view(1, 1, W)
    taps = []
    for k in range(9):
        i, j = divmod(k, 3)
        groups = []
        for g in range(G):
            ph = hh - 1 + i + off[..., 18 * g + 2 * k]
            pw = ww - 1 + j + off[..., 18 * g + 2 * k + 1]
            grid = torch.stack((2 * pw / (W - 1) - 1, 2 * ph / (H - 1) - 1), -1)
            s = F.grid_sample(xn[:, g * Cg:(g + 1) * Cg], grid, mode="bilinear", padding_mode="zeros",
                              align_corners=True)
            groups.append(s.permute(0, 2, 3, 1) * mask[..., 9 * g + k].unsqueeze(-1))
        taps.append(torch.cat(groups, -1))
    return torch.stack(taps, 3)


def conv_over_cols(cols, weight, bias):
    """y (N,H,W,Co) = bias + sum_{k,c} weight[co][c][i][j] * cols[k][c]."""
    Co, C = weight.shape[:2]
    return torch.einsum("nhwkc,ock->nhwo", cols, weight.reshape(Co, C, 9)) + bias


def conv_nine_1x1(cols, weight, bias):
    """The same product as nine 1x1 convolutions, one per tap (the second formulation's half of the conv)."""
    y = 0
    for k in range(9):
        i, j = divmod(k, 3)
        y = y + F.conv2d(cols[:, :, :, k].permute(0, 3, 1, 2), weight[:, :, i, j, None, None])
    return y.permute(0, 2, 3, 1) + bias


def dcn(x, off, mask, weight, bias, G, form="gather"):
    if form == "gather":
        return conv_over_cols(cols_gather(x, off, mask, G), weight, bias)
    return conv_nine_1x1(cols_grid(x, off, mask, G), weight, bias)


def split_om(om, G, sigmoid):
    """om (N,H,W,P >= 27G) -> (off, mask), the mask through the sigmoid when the channels hold logits."""
    off, m = om[..., :18 * G], om[..., 18 * G:27 * G]
    return off, (torch.sigmoid(m) if sigmoid else m)


def classify(off, H, W, G):
    """Fractions of (pixel, tap, group) samples with no corner inside, with some but not all of the corners they
    need (those of non-zero weight), and with all of them."""
    none = part = full = 0
    for g in range(G):
        for k in range(9):
            cs = corners(off, H, W, g, k)
            need = torch.stack([wt != 0 for _, _, wt, _, _ in cs])
            have = torch.stack([ok for _, ok, _, _, _ in cs])
            anyin = have.any(0)
            allneed = (have | ~need).all(0)
            none += (~anyin).sum().item()
            full += (anyin & allneed).sum().item()
            part += (anyin & ~allneed).sum().item()
    tot = float(none + part + full)
    return none / tot, part / tot, full / tot


def abs_terms_dom(dcols, x, off, mask, G):
    """Sum of absolute terms of the three offset/mask gradients, (N,H,W,27G) in om's channel order:
    |m| sum_c |dcol_c| sum_corners |d weight / d h| |x| (and d w), and sum_c |dcol_c| sum_corners weight |x|."""
    N, H, W, C = x.shape
    Cg = C // G
    out = torch.zeros(N, H, W, 27 * G, dtype=x.dtype)
    ax, ad, am = x.abs(), dcols.abs(), mask.abs()
    for g in range(G):
        xg = ax[..., g * Cg:(g + 1) * Cg].reshape(N, H * W, Cg)
        for k in range(9):
            d = ad[:, :, :, k, g * Cg:(g + 1) * Cg]
            sh = sw = sv = 0
            for idx, ok, wt, dh, dw in corners(off, H, W, g, k):
                v = (d * _take(xg, idx)).sum(-1) * ok
                sh, sw, sv = sh + dh.abs() * v, sw + dw.abs() * v, sv + wt * v
            out[..., 18 * g + 2 * k] = am[..., 9 * g + k] * sh
            out[..., 18 * g + 2 * k + 1] = am[..., 9 * g + k] * sw
            out[..., 18 * G + 9 * g + k] = sv
    return out


def dx_counts(off, x_shape, G):
    """n_e: how many (pixel, tap, corner) contributions with a non-zero weight land on each element of dx (N,H,W,C)."""
    N, H, W, C = x_shape
    Cg = C // G
    out = torch.zeros(N, H * W, C, dtype=torch.float64)
    for g in range(G):
        for k in range(9):
            for idx, ok, wt, _, _ in corners(off, H, W, g, k):
                hit = (ok & (wt != 0)).to(torch.float64).reshape(N, -1, 1).expand(-1, -1, Cg)
                out[..., g * Cg:(g + 1) * Cg].scatter_add_(1, idx.reshape(N, -1, 1).expand(-1, -1, Cg), hit)
    return out.view(N, H, W, C)


def draw_offsets(gen, N, H, W, G, grad):
    """The offset draw of every kernel test: integer part uniform in [-2, 2], fraction j/8 with j in 0..7 (forward
    tests: exact integer coordinates occur) or 1..7 (gradient tests: no sample on a kink of the bilinear map), and one
    (pixel, tap) in 16 replaced by +-(H+3, W+3).  Every value is exact in bf16.  float64 (N,H,W,18G)."""
    shape = (N, H, W, 9 * G, 2)
    whole = torch.randint(-2, 3, shape, generator=gen).double()
    frac = torch.randint(1 if grad else 0, 8, shape, generator=gen).double() / 8
    off = whole + frac
    far = torch.randint(0, 16, shape[:-1], generator=gen) == 0
    sign = torch.randint(0, 2, shape[:-1], generator=gen).double() * 2 - 1
    big = torch.stack((sign * (H + 3), sign * (W + 3)), -1)
    off = torch.where(far.unsqueeze(-1), big, off)
    # (tap, (dh, dw)) pairs of a group are channels 18g + 2k, 18g + 2k + 1
    return off.view(N, H, W, 18 * G)
