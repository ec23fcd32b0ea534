"""Float64 references of the convolutional core and the one checker the per-layer GPU tests use
(tests/test_conv_layers_gpu.py: the Nature network, trunk.hip and qnet.hip; tests/test_cnn_layers_gpu.py:
the reference ``cnn``, cnn.hip). CPU code: nothing here touches a GPU.

Layouts. Activations are NHWC; a conv weight is [K][N] with k = (kh, kw, ci) (the flat buffer's HWIO
tensor seen as a matrix, as tests/test_wgrad_tiles_gpu.py has it). Every reference returns the value
and S, the same sum with every term replaced by its absolute value (|x| |w| scale + |b| forward,
|dz| |w| backward): the scale of the rounding error of any summation order.

What a per-layer test leaves to bound. Each layer is fed the kernel's own stored previous tensor (or a
test-made one), exact in the build's storage type, and the reference is formed in float64 from the same
stored values, so nothing propagates from layer to layer. What is left:

  products      16-bit builds: bf16 x bf16 (16 significand bits) and fp16 x fp16 (22) are exact in
                fp32, and so is u8 x 16-bit. fp32 build: the fp32 MFMA may round each product: one
                rounding (extra_roundings + 1). Its fused conv1 (trunk.hip, cnn.hip: split3_bf16)
                splits every fp32 weight into three bf16 parts h + m + l == w exactly and runs three
                bf16 MFMAs against the u8 pixels: exact products, three times the terms (terms = 3 K),
                and |h| + |m| + |l| <= (1 + 2^-6) |w|, which ``SPLIT3_S`` puts on S.
  additions     a sum of ``terms`` products in ANY order -- the MFMA's internal adder tree, the k-steps
                in sequence, the K range split across the wave halves of a block and met in LDS (igemm
                KSPLIT 2 / 4, dgrad_s2's two halves, the fused trunks' park / unpark, cnn_bwd's four
                parts) -- passes each product through at most terms - 1 inexact fp32 additions (adding
                to an exact zero, which is what a padding tap, an invalid dgrad tap and a masked A row
                contribute, is exact). Each has relative error <= 2^-23 whatever the adder's rounding
                mode (2^-24 if it rounds to nearest; the ulp covers truncation), so to first order
                |err| <= (terms - 1) 2^-23 S. The K split changes the order, not the count.
  epilogue      forward: v * scale (one rounding; counted even where scale == 1) and + bias (one
                rounding, |bias| is part of S): extra_roundings = 2. dgrad: the ReLU mask selects, no
                arithmetic: 0. With the one the additions leave spare, (terms + extra_roundings) 2^-23 S
                bounds the fp32 value before the store, second-order terms included at these sizes
                ((1 + 2^-23)^3000 - 1 < 1.0002 x 3000 x 2^-23).
  loss scale    the fp16 build's dH / dz carry kLossScale = 1024, a power of two: the stored values are
                what the references read, so it appears nowhere.
  storage       one float -> act_t conversion of the fp32 value. csrc/kernels/common.h and fused_util.h
                convert with a plain C++ cast ``(act_t)v`` (pack4, the igemm epilogues, pool_bwd8):
                round-to-nearest-even for __bf16 and _Float16 alike (f2bf says so for the bf16 helper;
                the cast lowers to v_cvt_pk_bf16_f32 / v_cvt_f16_f32 under the default rounding mode).
                It does not truncate, so u is the UNIT ROUNDOFF, half an ulp: 2^-8 (bf16: 8 significand
                bits), 2^-11 (fp16), 2^-24 (fp32: the "conversion" is the identity; kept for uniformity).
                Below the smallest normal number the spacing stops shrinking, so the relative term is
                taken of max(|ref| + e, smallest normal): the only case it matters is fp16 (2^-14).

``check`` therefore asserts, per element and with no element excluded,

    |out - ref| <= e + u * max(|ref| + e, tiny),    e = (terms + extra_roundings) * 2^-23 * S

ReLU needs no exception: |relu(a) - relu(b)| <= |a - b|, so the bound on the pre-activation holds for the
activation, with ref = relu(pre-activation). A masked dgrad element has ref == S == 0 and must be exactly 0
(u * tiny is below the smallest subnormal of every type).

Max-pool (2x2 / stride 2, SAME: the padding is at the bottom and right only, and never wins). Forward:
the maximum of stored values is one of them: bit-exact. Backward: the gradient goes to the FIRST maximum
in row-major order within the window (the rule cnn.hip pool_bwd8 states), and only where that maximum is
> 0 (the ReLU before the pool); written with an explicit scan, not through torch.max_pool2d.
"""
import torch

EPS = 2.0 ** -23
# storage type -> (unit roundoff of the round-to-nearest-even float -> act_t cast, smallest normal)
UNIT = {torch.bfloat16: (2.0 ** -8, 2.0 ** -126), torch.float16: (2.0 ** -11, 2.0 ** -14),
        torch.float32: (2.0 ** -24, 2.0 ** -126)}
SPLIT3_S = 1.0 + 2.0 ** -6      # |h| + |m| + |l| <= SPLIT3_S |w| for the three bf16 parts of an fp32 w


def same_pads(n, k, s):
    """(before, after) of TF SAME padding for n inputs, kernel k, stride s."""
    total = max(((n + s - 1) // s - 1) * s + k - n, 0)
    return total // 2, total - total // 2


# ------------------------------------------------------------------ convolution as explicit GEMMs
def patches(x, k, stride, pads=(0, 0, 0, 0)):
    """x [B][IH][IW][C] -> A [B * OH * OW][k * k * C], k = (kh, kw, ci), of the input zero-padded by
    pads = (top, bottom, left, right); and (OH, OW)."""
    B, IH, IW, C = x.shape
    pt, pb, pl, pr = pads
    xp = torch.zeros(B, IH + pt + pb, IW + pl + pr, C, dtype=torch.float64)
    xp[:, pt:pt + IH, pl:pl + IW] = x
    u = xp.unfold(1, k, stride).unfold(2, k, stride)            # [B][OH][OW][C][kh][kw]
    OH, OW = u.shape[1], u.shape[2]
    return u.permute(0, 1, 2, 4, 5, 3).reshape(B * OH * OW, k * k * C), (OH, OW)


def dgrad_patches(dz, k, stride, in_hw, pads=(0, 0)):
    """dz [B][OH][OW][CO] -> A [B * IH * IW][k * k * CO], k = (kh, kw, co): A[(b, iy, ix)][(kh, kw, co)] =
    dz[b][oy][ox][co] where iy + top - kh == stride * oy and ix + left - kw == stride * ox, else 0
    (pads = (top, left): the rows below and right of the input never reach an input pixel)."""
    B, OH, OW, CO = dz.shape
    (IH, IW), (pt, pl) = in_hw, pads
    A = torch.zeros(B, IH, IW, k, k, CO, dtype=torch.float64)
    for kh in range(k):
        for kw in range(k):
            for oy in range(OH):
                iy = stride * oy + kh - pt
                if not 0 <= iy < IH:
                    continue
                for ox in range(OW):
                    ix = stride * ox + kw - pl
                    if 0 <= ix < IW:
                        A[:, iy, ix, kh, kw] = dz[:, oy, ox]
    return A.reshape(B * IH * IW, k * k * CO)


def dgrad_weights(w, k, cin, cout):
    """w [k * k * cin][cout] -> [k * k * cout][cin]: row (tap, co), column ci."""
    return w.reshape(k * k, cin, cout).permute(0, 2, 1).reshape(k * k * cout, cin)


def gemm(A, W):
    """(A W, |A| |W|) in float64."""
    return A @ W, A.abs() @ W.abs()


def conv_fwd(x, w, b, k, stride, pads=(0, 0, 0, 0), scale=1.0, relu=True):
    """relu(scale * conv(x, w) + b) -> ([B][OH][OW][N], S) with S = scale |x| * |w| + |b|."""
    A, (OH, OW) = patches(x, k, stride, pads)
    y, S = gemm(A, w)
    y, S = y * scale + b, S * abs(scale) + b.abs()
    if relu:
        y = y.clamp_min(0.0)
    shape = (x.shape[0], OH, OW, w.shape[1])
    return y.reshape(shape), S.reshape(shape)


def conv_dgrad(dz, w, k, stride, x_in, pads=(0, 0), mask=True):
    """d(conv input) = (dz * w^T) * (x_in > 0), x_in [B][IH][IW][CIN] the layer input (its ReLU mask;
    mask False: no mask) -> ([B][IH][IW][CIN], S)."""
    B, IH, IW, cin = x_in.shape
    A = dgrad_patches(dz, k, stride, (IH, IW), pads)
    d, S = gemm(A, dgrad_weights(w, k, cin, dz.shape[3]))
    d, S = d.reshape(x_in.shape), S.reshape(x_in.shape)
    if mask:
        keep = (x_in > 0).double()
        d, S = d * keep, S * keep
    return d, S


def dense_dgrad(dh, w, x_in):
    """(dh w^T) * (x_in > 0): dh [B][H], w [F][H], x_in [B][F] -> ([B][F], S)."""
    d, S = gemm(dh, w.t())
    keep = (x_in > 0).double()
    return d * keep, S * keep


# ------------------------------------------------------------------ 2x2 / stride-2 SAME max-pool
def _windows(a):
    """a [B][H][W][C] -> v [4][B][QH][QW][C] (cell i = (dy, dx) = (i >> 1, i & 1), row-major; cells
    outside the map hold -inf) and valid [4][QH][QW]."""
    B, H, W, C = a.shape
    QH, QW = (H + 1) // 2, (W + 1) // 2
    ap = torch.full((B, 2 * QH, 2 * QW, C), float('-inf'), dtype=torch.float64)
    ap[:, :H, :W] = a
    inside = torch.zeros(2 * QH, 2 * QW, dtype=torch.bool)
    inside[:H, :W] = True
    v = torch.stack([ap[:, (i >> 1)::2, (i & 1)::2] for i in range(4)])
    return v, torch.stack([inside[(i >> 1)::2, (i & 1)::2] for i in range(4)])


def pool_argmax(a):
    """Per window and channel: (the maximum over the cells inside the map, the index 0..3 of the FIRST
    cell in row-major order that attains it). Explicit scan with a strict comparison."""
    v, valid = _windows(a)
    best = torch.full(v.shape[1:], float('-inf'), dtype=torch.float64)
    arg = torch.zeros(v.shape[1:], dtype=torch.int64)
    for i in range(4):
        better = valid[i][None, :, :, None] & (v[i] > best)
        best = torch.where(better, v[i], best)
        arg = torch.where(better, torch.full_like(arg, i), arg)
    return best, arg


def pool_fwd(a):
    """[B][H][W][C] -> [B][ceil(H / 2)][ceil(W / 2)][C]."""
    return pool_argmax(a)[0]


def pool_bwd(a, dp):
    """dp [B][QH][QW][C] routed to the first maximum of each window of a, where that maximum is > 0;
    zero elsewhere. Returns the shape of a."""
    B, H, W, C = a.shape
    best, arg = pool_argmax(a)
    QH, QW = best.shape[1], best.shape[2]
    out = torch.zeros(B, 2 * QH, 2 * QW, C, dtype=torch.float64)
    live = best > 0
    for i in range(4):
        out[:, (i >> 1)::2, (i & 1)::2] = torch.where((arg == i) & live, dp, torch.zeros_like(dp))
    return out[:, :H, :W].contiguous()


# ------------------------------------------------------------------ the checker
def check(out, ref, S, terms, act_dtype, extra_roundings=0, tag=''):
    """Asserts |out - ref| <= e + u max(|ref| + e, tiny) with e = (terms + extra_roundings) 2^-23 S for
    EVERY element (module docstring); returns the largest err / bound."""
    u, tiny = UNIT[act_dtype]
    out, ref, S = out.double().cpu(), ref.double(), S.double()
    assert out.shape == ref.shape == S.shape, (tag, out.shape, ref.shape, S.shape)
    assert bool(torch.isfinite(out).all()), '%s: an element was left unwritten (or is not finite)' % tag
    e = (terms + extra_roundings) * EPS * S
    bound = e + u * (ref.abs() + e).clamp_min(tiny)
    err = (out - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), (tag, '%d of %d elements' % (int(bad.sum()), bad.numel()),
                                 [(idx.tolist(), float(out[tuple(idx)]), float(ref[tuple(idx)]), float(bound[tuple(idx)]))
                                  for idx in bad.nonzero()[:5]])
    return float((err / bound).max())
