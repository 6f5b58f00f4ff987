"""A numpy model of the F16X3 operand planes (diff3dhpe_amd/csrc/weight_pack.hip, d3d_kernels.h): what a kernel that follows its design
computes from fp32 operands, with the accumulation done exactly (fp64) -- so a kernel's distance to this model is its accumulation and
epilogue rounding alone, whatever exponent the weight planes carry, and the model's own distance to the exact product is the part of
the error the planes are responsible for (the "floor" of a weight exponent k).

  weight planes      hi = fp16(s), lo = fp16(s - hi) of s = 2^k w, k per matrix (weight_exp)
  activation planes  the same of s = 8 x
  product            a_hi w_hi + a_hi w_lo + a_lo w_hi, un-scaled by 2^-(3 + k)

Plain module (no fixtures, no GPU): the host tests check the model against itself, the GPU tests check the kernels against it."""
import numpy as np

HALF_MAX = 65504.0
K_MAX, K_MIN = 12, -14
MIN_WEIGHT_EXP = 0          # F16X3_MIN_WEIGHT_EXP of weight_pack.h: the commit refuses a matrix whose exponent is lower
A_SCALE = 8.0


def weight_exp(W):
    """split_weight_f16x3's exponent: the largest k <= 12 with fl32(amax 2^k) <= 65504 over the finite entries, floor -14."""
    w = np.abs(np.asarray(W, dtype=np.float32)).ravel()
    w = w[w <= np.float32(3.0e38)]
    amax = np.float32(w.max()) if w.size else np.float32(0.0)
    k = K_MAX
    with np.errstate(over="ignore"):
        while k > K_MIN and np.ldexp(amax, k).astype(np.float32) > np.float32(HALF_MAX):
            k -= 1
    return k


def split(x, scale):
    """(hi, lo) planes of scale * x as float64 arrays: s = fl32(scale x) clamped to +-65504, hi = fp16(s) and lo = fp16(fl32(s - hi)), both
    round-to-nearest-even (numpy's float32 -> float16 conversion)."""
    with np.errstate(over="ignore", under="ignore"):
        s = np.asarray(x, dtype=np.float32) * np.float32(scale)
        s = np.clip(s, np.float32(-HALF_MAX), np.float32(HALF_MAX))
        hi = s.astype(np.float16)
        lo = (s - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def split_weight(W):
    """(hi, lo, k) of a weight matrix at its own exponent."""
    k = weight_exp(W)
    hi, lo = split(W, np.ldexp(1.0, k))
    return hi, lo, k


def gemm(A, W):
    """The three products of A [M, K] and W [N, K] on their planes, summed in fp64: (8 2^k) A W^T up to the planes' error.  Un-scaled."""
    ah, al = split(A, A_SCALE)
    wh, wl, _ = split_weight(W)
    return ah @ wh.T + ah @ wl.T + al @ wh.T


def product(A, W):
    """gemm(A, W) with the kernels' out_scale 2^-(3 + k) applied: the model's A W^T."""
    return gemm(A, W) * np.ldexp(1.0, -(3 + weight_exp(W)))


def exact(A, W):
    return np.asarray(A, dtype=np.float64) @ np.asarray(W, dtype=np.float64).T


def floor(A, W, skip_cols=()):
    """max |product - exact| over the output columns not listed in skip_cols: what the planes cost at this matrix's exponent."""
    d = np.abs(product(A, W) - exact(A, W))
    keep = np.ones(d.shape[1], dtype=bool)
    keep[list(skip_cols)] = False
    return float(d[:, keep].max())


def fold_layernorm(W, b, gamma, beta):
    """fold_layernorm of weight_pack.hip: wg = fl32(W gamma) [N, K], csum[n] = sum_q wg[n, q] and fb[n] = b[n] + sum_q W[n, q] beta[q] summed
    in fp64 and rounded to fp32.  LN(x) W^T + b = rstd (x wg^T) - rstd mean csum + fb."""
    W32, g32 = np.asarray(W, dtype=np.float32), np.asarray(gamma, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore"):
        wg = W32 * g32[None, :]
    csum = wg.astype(np.float64).sum(axis=1).astype(np.float32)
    fb = (np.asarray(b, dtype=np.float64) + W32.astype(np.float64) @ np.asarray(beta, dtype=np.float64)).astype(np.float32)
    return wg, csum, fb


def folded_linear(x, W, b, gamma, beta, eps):
    """LN(x; gamma, beta, eps) W^T + b the way the folded GEMMs compute it, on the planes of x and of wg, everything else in fp64.
    Returns (result, k of the folded matrix)."""
    wg, csum, fb = fold_layernorm(W, b, gamma, beta)
    xd = np.asarray(x, dtype=np.float64)
    mean = xd.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(xd.var(axis=1, keepdims=True) + eps)
    acc = product(x, wg)
    return rstd * (acc - mean * csum.astype(np.float64)[None, :]) + fb.astype(np.float64)[None, :], weight_exp(wg)


# ---- the same on torch tensors (any device): the GPU tests model matrices of 10^5 rows, which numpy would take seconds for.
# torch's float32 -> float16 conversion rounds to nearest even on every backend; test_plane_model_host.py pins the two forms to each other.
def split_t(x, scale):
    import torch
    s = (x.to(torch.float32) * float(scale)).clamp(-HALF_MAX, HALF_MAX)
    hi = s.to(torch.float16)
    lo = (s - hi.to(torch.float32)).to(torch.float16)
    return hi.double(), lo.double()


def product_t(A, W):
    """product() on torch tensors: (A W^T of the model as float64 on A's device, k)."""
    k = weight_exp(W.detach().cpu().numpy())
    ah, al = split_t(A, A_SCALE)
    wh, wl = split_t(W, 2.0 ** k)
    return (ah @ wh.t() + ah @ wl.t() + al @ wh.t()) * 2.0 ** -(3 + k), k


def folded_linear_t(x, W, b, gamma, beta, eps):
    """folded_linear() on torch tensors (the fold itself on the host, as the commit does it): (result, k of the folded matrix)."""
    import torch
    wg, csum, fb = fold_layernorm(W.detach().cpu().numpy(), b.detach().cpu().numpy(), gamma.detach().cpu().numpy(), beta.detach().cpu().numpy())
    dev = x.device
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + eps)
    acc, k = product_t(x, torch.from_numpy(wg).to(dev))
    return rstd * (acc - mean * torch.from_numpy(csum).to(dev).double()) + torch.from_numpy(fb).to(dev).double(), k


def outlier_for(k):
    """A weight value that alone puts a matrix of ordinary entries at exponent k: 3/4 of the way up k's interval of amax."""
    assert K_MIN <= k <= K_MAX
    return float(np.float32(0.75 * HALF_MAX * 2.0 ** -k))
