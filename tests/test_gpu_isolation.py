"""Row isolation on the MI355X: a row's (group's, batch element's) result depends on that row's own inputs only, and a launch writes its
own output only.

A. op level: every hook once on clean rows and once with every odd row / attention group made NaN or +Inf -- the clean rows must come
   out bit for bit as before (a masked key still enters the second product as 0 x V; 0 x NaN is NaN).
B. engine level: one batch element poisoned; the others must be bit-identical to the clean call, and the poisoned one must never come
   back finite with a clean guard word.
C. guard bands: the C ABI called directly with every output (and fp32 input, and the workspace) inside a NaN-patterned band.

Every comparison is torch.equal or bit-pattern equality: there are no tolerances here.  The helpers (helpers.banded, untouched,
group_index, poison_groups) have CPU self-tests in tests/test_isolation_helpers_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import hashed, torch_sd, inputs, cfg_full, banded, untouched, group_index, poison_groups
from diff3dhpe_amd import _lib
from diff3dhpe_amd.spec import DenoiserConfig

gpu = pytest.mark.gpu
D, H = 512, 8


# ------------------------------------------------------------------------------------------------ A. op level
def _E():
    from diff3dhpe_amd import engine
    return engine


def _isolated(clean, bad, keep, own_fp32):
    """clean / bad: the results (or tuples of results, rows first) of the clean and the poisoned call."""
    keep = keep.to(clean[0].device if isinstance(clean, tuple) else clean.device)
    for c, b in zip(*(r if isinstance(r, tuple) else (r,) for r in (clean, bad))):
        if c is None:
            continue
        assert torch.isfinite(c).all()
        same = (c[keep].view(torch.int32) == b[keep].view(torch.int32)).reshape(int(keep.sum()), -1).all(1)
        assert same.all(), f"{int((~same).sum())} clean rows changed, the first is row {int(keep.nonzero().flatten()[(~same).nonzero()[0, 0]])}"
        if own_fp32:
            assert not torch.isfinite(b[~keep]).any(), "a poisoned row came back with finite values"


def _lin_operands(M, N, K):
    A = hashed(f"isoA{M}", (M, K), 11, 2.0).cuda()
    W = hashed(f"isoW{N}_{K}", (N, K), 12, 1.0 / np.sqrt(K)).cuda()
    b = hashed(f"isob{N}", (N,), 13, 0.5).cuda()
    R = (hashed(f"isoR{M}", (M, N), 14, 1.5) + 0.3).cuda()
    return A, W, b, R


def _odd_rows(A):
    return poison_groups(A, torch.arange(A.shape[0]))


LINEAR = [(300, 512, 512, p, e) for p in ("fp32", "f16x3", "bf16") for e in ("none", "gelu", "residual")]
LINEAR += [(129, 130, 96, p, e) for p in ("fp32", "f16x3") for e in ("none", "gelu", "residual")]      # the on-the-fly-split kernel
LINEAR += [(66100, 512, 512, "f16x3", "gelu")]                                      # the persistent walk, ragged last tile, row slices


@gpu
@pytest.mark.parametrize("M,N,K,prec,epi", LINEAR)
def test_a1_linear_rows(M, N, K, prec, epi):
    A, W, b, R = _lin_operands(M, N, K)
    bad, keep = _odd_rows(A)
    run = lambda a: _E().op_linear(a, W, b, residual=R if epi == "residual" else None, epi=epi, precision=prec)
    _isolated(run(A), run(bad), keep, own_fp32=prec == "fp32")


def _row_classes(M, N):
    rpb = 51
    return dict(pos=hashed("isopos", (9, N), 27, 0.5).cuda(), pos_div=17, tvec=hashed("isotv", ((M + rpb - 1) // rpb, N), 29, 0.5).cuda(),
                rows_per_batch=rpb)


def _gb(N):
    return (1 + 0.2 * hashed("isog", (N,), 25)).cuda(), (0.2 * hashed("isobe", (N,), 26)).cuda()


@gpu
@pytest.mark.parametrize("with_stats", [False, True])
def test_a1_linear_postnorm_rows(with_stats):
    M, N, K = 300, 512, 512
    A, W, b, R = _lin_operands(M, N, K)
    g, be = _gb(N)
    bad, keep = _odd_rows(A)
    run = lambda a: _E().op_linear_postnorm(a, W, b, R, g, be, 1e-6, with_stats=with_stats, **_row_classes(M, N))[:2]
    _isolated(run(A), run(bad), keep, own_fp32=False)


@gpu
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("op", ["postnorm", "postnorm_stats", "residual", "gelu"])
def test_a1_splitk_rows(op, S):
    E = _E()
    M, K = 130, 512
    N = 1024 if op == "gelu" else 512
    A, W, b, R = _lin_operands(M, N, K)
    bad, keep = _odd_rows(A)
    if op == "gelu":
        g, be = _gb(K)
        run = lambda a: E.op_linear_splitk_gelu(a, W, b, g, be, 1e-6, S=S)[:1]
    elif op == "residual":
        run = lambda a: E.op_linear_splitk_residual(a, W, b, R, S=S, with_stats=True)[:2]
    else:
        g, be = _gb(N)
        run = lambda a: E.op_linear_splitk_postnorm(a, W, b, R, g, be, 1e-6, S=S, with_stats=op == "postnorm_stats", **_row_classes(M, N))[:2]
    _isolated(run(A), run(bad), keep, own_fp32=False)


@gpu
def test_a1_layernorm_rows():
    x = hashed("isolnx", (333, 512), 3, 3.0).cuda() + 0.7
    g, be = _gb(512)
    bad, keep = _odd_rows(x)
    _isolated(_E().op_layernorm(x, g, be, 1e-6), _E().op_layernorm(bad, g, be, 1e-6), keep, own_fp32=True)


def _head_engine():
    from diff3dhpe_amd.engine import Engine
    cfg = DenoiserConfig(num_frame=27, embed_dim=512, depth=2)
    eng = Engine(cfg, precision="f16x3")
    eng.load_weights(torch_sd(cfg, 11))
    return eng


@gpu
@pytest.mark.parametrize("rows", [33, 4131])
def test_a1_head_rows(rows):
    eng = _head_engine()
    X = hashed(f"isohead{rows}", (rows, 512), 12, 1.7).cuda() + 0.3
    bad, keep = _odd_rows(X)
    _isolated(eng.head(X), eng.head(bad), keep, own_fp32=True)


# (B, T, J, D, temporal, precision, generic)
ATTN = [(2, 5, 17, 512, False, "fp32", False), (2, 5, 17, 512, False, "fp32", True), (2, 9, 17, 32, False, "fp32", False)]
ATTN += [(B, T, J, 512, True, p, gen) for (B, T, J) in ((2, 81, 3), (1, 243, 2)) for p in ("fp32", "f16x3") for gen in (False, True)]
ATTN += [(2, 27, 17, 512, False, "bf16", False), (2, 27, 17, 512, True, "bf16", False)]
ATTN += [(8, 243, 17, 512, True, "f16x3", False), (8, 230, 17, 512, True, "f16x3", False),      # staggered persistent temporal kernel
         (24, 81, 17, 512, True, "f16x3", False),                                               # persistent 3-tile kernel
         (3 * 243, 17, 1, 512, True, "f16x3", False)]                                           # wave-private persistent spatial kernel


@gpu
@pytest.mark.parametrize("what", ["rows", "v_only"])
@pytest.mark.parametrize("B,T,J,Dm,temporal,prec,generic", ATTN)
def test_a2_attention_groups(B, T, J, Dm, temporal, prec, generic, what):
    """what = v_only: the odd groups keep finite q and k, so their own softmax is finite and only a `0 x NaN` product can leak."""
    qkv = hashed(f"isoqkv{T}_{J}_{Dm}_{B}", (B * T * J, 3 * Dm), 21, 2.0).cuda()
    bad, keep = poison_groups(qkv, group_index(B, T, J, temporal), cols=slice(2 * Dm, 3 * Dm) if what == "v_only" else None)
    run = lambda x: _E().op_attention(x, B, T, J, H, temporal, precision=prec, force_generic=generic)
    # fp32 results are the kernel's own; f16x3 temporal and bf16 results come back through a conversion of clamped planes.  The f16x3
    # fast path also gets its INPUT through a clamp (k_split_qkv): the poisoned groups reach the kernel as +-65504, so these cases
    # check the masking of huge finite neighbours; NaN / Inf planes reach the same kernels in part B (LARGE)
    own = prec == "fp32" or (prec == "f16x3" and (generic or not temporal))
    _isolated(run(qkv), run(bad), keep, own_fp32=own)


# ------------------------------------------------------------------------------------------------ B. engine level
_SD = {}


def _sd(cfg):   # cached per (num_frame, seq2frame): every engine of this module loads the same seed-21 weights
    key = (cfg.num_frame, cfg.seq2frame)
    if key not in _SD:
        _SD[key] = torch_sd(cfg, 21)
    return _SD[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_weights():
    yield
    _SD.clear()


def _engine(cfg, prec, opts=()):
    from diff3dhpe_amd.engine import Engine
    from oracle import d3d_oracle as orc
    eng = Engine(cfg, precision=prec)
    eng.load_weights(_sd(cfg))
    for k, v in opts:
        eng.set_option(k, v)
    tabs = orc.diffusion_tables("cosine", 1000)
    eng.set_schedule(tabs["alphas_cumprod"], tabs["sqrt_one_minus_alphas_cumprod"], 3, 0.0, True)
    return eng


MODES = {"fp32": ("fp32", ()), "bf16": ("bf16", ()), "f16x3": ("f16x3", ()),
         "f16x3-two-kernel-attention": ("f16x3", (("fused_spatial", 0), ("fused_temporal", 0))),
         "f16x3-row-postnorm": ("f16x3", (("fused_postnorm", 0),)),
         "f16x3-row-layernorm": ("f16x3", (("fold_layernorm", 0),))}
# T, seq2frame, B, poisoned batch elements
SHAPES = {"T27": (27, False, 5, (1, 3)), "T81": (81, False, 3, (1,)), "T243": (243, False, 3, (1,)), "s2f_T27": (27, True, 3, (1,))}
POISONS = ("x2d_one_nan", "x2d_all_inf", "y_one_nan")


def _poisoned(x2d, y, which, poison):
    x2d, y = x2d.clone(), y.clone()
    for b in which:
        if poison == "x2d_one_nan":
            x2d[b, 3, 5, 0] = float("nan")
        elif poison == "x2d_all_inf":
            x2d[b] = float("inf")
        else:
            y[b, min(3, y.shape[1] - 1), 5, 0] = float("nan")
    return x2d, y


def _plan(eng):
    return {k: eng.info(k) for k in ("proj_split_last", "fc1_split_last", "fc2_split_last", "bf16_fused_spatial_last", "bf16_fused_temporal_last")}


def _check_batch_isolation(eng, prec, T, s2f, B, which, want_plan, graph=False):
    """The body of every part B test; returns nothing, raises one AssertionError that lists every failed case."""
    inp = inputs(B, T, 310)
    x2d = inp["x2d"].cuda()
    y = (inp["noise"][:, :1] if s2f else inp["noise"]).contiguous().cuda()
    t = torch.tensor([(431 * i + 77) % 1000 for i in range(B)], dtype=torch.float32, device="cuda")
    clean_rows = torch.tensor([b not in which for b in range(B)], device="cuda")
    failures = []

    def plan_ok(call):
        got = _plan(eng)
        if isinstance(want_plan["fc2_split_last"], tuple):
            ok = got["fc2_split_last"] in want_plan["fc2_split_last"] and all(got[k] == v for k, v in want_plan.items() if k != "fc2_split_last")
        else:
            ok = got == want_plan
        if not ok:
            failures.append(f"{call}: ran plan {got}, the case names {want_plan}")

    eng.range_flags(clear=True)
    den0 = eng.denoise(x2d, y, t).clone()
    plan_ok("denoise")
    ddim0 = eng.ddim_sample(x2d, y).clone()
    plan_ok("ddim_sample")
    assert torch.isfinite(den0).all() and torch.isfinite(ddim0).all()
    assert eng.range_flags(clear=True) == 0
    for poison in POISONS:
        bx, by = _poisoned(x2d, y, which, poison)
        den = eng.denoise(bx, by, t)
        flags = eng.range_flags(clear=True)
        if not torch.equal(den[clean_rows], den0[clean_rows]):
            failures.append(f"denoise, {poison}: a clean batch element changed")
        finite = torch.isfinite(den[~clean_rows])
        if prec == "f16x3":
            if finite.any() and not flags & _lib.RANGE_PRECISION:
                failures.append(f"denoise, {poison}: SILENT -- {int(finite.sum())} of {finite.numel()} values of the poisoned elements are "
                                f"finite and the guard word is {flags:#x}")
        elif finite.any():
            failures.append(f"denoise, {poison}: {int(finite.sum())} of {finite.numel()} values of the poisoned elements are finite")
        runs = [("ddim_sample", False)] + ([("ddim_sample under graph replay", True)] if graph else [])
        for name, g in runs:
            eng.set_graph_mode(g)
            try:
                out = eng.ddim_sample(bx, by)
            finally:
                eng.set_graph_mode(False)
            if not torch.equal(out[clean_rows], ddim0[clean_rows]):
                failures.append(f"{name}, {poison}: a clean batch element changed")
        eng.range_flags(clear=True)
    assert not failures, "\n".join(failures)


def _want_plan(prec, splits=(0, 0, 0)):
    bf = int(prec == "bf16")
    return {"proj_split_last": splits[0], "fc1_split_last": splits[1], "fc2_split_last": splits[2], "bf16_fused_spatial_last": bf,
            "bf16_fused_temporal_last": bf}


@gpu
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_b_poisoned_batch_element(shape, mode):
    """1. every clean batch element is torch.equal to the same element of the clean call (denoise, and a 3-step ddim_sample with eta 0
    and clipping; the F16X3 default at T = 27 once more under graph replay); 2. denoise never returns a poisoned element finite with a
    clean guard word (fp32, bf16: it is entirely non-finite)."""
    T, s2f, B, which = SHAPES[shape]
    prec, opts = MODES[mode]
    eng = _engine(cfg_full(T, seq2frame=s2f), prec, opts)
    _check_batch_isolation(eng, prec, T, s2f, B, which, _want_plan(prec), graph=(mode == "f16x3" and shape == "T27"))


# Batches large enough for the forms the small ones never select, with real NaN / Inf planes from the qkv GEMM epilogue (the op hook of
# part A2 converts fp32 to planes with a clamp: its F16X3 fast-path cases see finite neighbours only).  One stream, so that ddim_sample
# runs the whole batch in one carve-up as denoise does.  T, mode, B:
#   two-kernel attention, B J H >= 1024: the staggered persistent temporal kernel (T = 243: 13 pad rows) and the persistent 3-tile
#     kernel (T = 81: 15); B T H >= 4096: the wave-private spatial kernel k_attn_temporal_x3p<1, 8>;
#   two-kernel attention, T = 27, B J H >= 4096: the wave-private temporal kernel k_attn_temporal_x3p<1, 6, 4> (5 pad rows);
#   default flow, T = 243, B = 16: launch_proj_x3 (>= 512 tiles of 192 x 256) and launch_fc1_x3 (>= 512 tiles of 256 x 256), whose
#     tiles cross the batch boundaries, beside the fused attention kernels at several tiles per workgroup.
LARGE = [(243, "f16x3-two-kernel-attention", 8), (81, "f16x3-two-kernel-attention", 8), (27, "f16x3-two-kernel-attention", 32),
         (243, "f16x3", 16)]


@gpu
@pytest.mark.parametrize("T,mode,B", LARGE)
def test_b_poisoned_batch_elements_large_batch(T, mode, B):
    """Every odd batch element poisoned: each clean one has poisoned neighbours on both sides (the last one: in front)."""
    prec, opts = MODES[mode]
    M, J = B * T * 17, 17
    if opts:
        assert B * J * H >= (4096 if T <= 32 else 1024) and B * T * H >= 4096
    else:
        assert (M // 192) * (D // 256) >= 512 and ((M + 255) // 256) * (2 * D // 256) >= 512
    eng = _engine(cfg_full(T), prec, opts + (("streams", 1),))
    _check_batch_isolation(eng, prec, T, False, B, tuple(range(1, B, 2)), _want_plan(prec))


@gpu
@pytest.mark.parametrize("S", [2, 4])
def test_b_poisoned_batch_element_latency_mode(S):
    eng = _engine(cfg_full(27), "f16x3", (("latency_mode", 1), ("proj_split", S), ("fc1_split", S)))
    _check_batch_isolation(eng, "f16x3", 27, False, 2, (1,), _want_plan("f16x3", (S, S, (2, 4))))


# ------------------------------------------------------------------------------------------------ C. guard bands
def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_ALIVE = []


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    _ALIVE.clear()


def _in(t):
    """An fp32 input the kernels read directly, inside NaN bands: a read outside it shows in the result.  The copy lives until the test
    ends (the ABI gets a bare address: a temporary would hand its block back to the allocator before the launch)."""
    if t is None:
        return None
    v, _ = banded(tuple(t.shape))
    v.copy_(t)
    _ALIVE.append(v)
    return v


class _Outs:
    """The guarded outputs of one ABI call."""

    def __init__(self):
        self.items = []

    def new(self, shape, name, written=True, dtype=torch.float32):
        v, check = banded(shape, dtype=dtype)
        self.items.append((name, v, check, written))
        return v

    def verify(self, want):
        """want: {name: the wrapper's result from ordinary tensors}."""
        torch.cuda.synchronize()
        for name, v, check, written in self.items:
            check()
            if written:
                assert untouched(v) == 0, f"{name}: {untouched(v)} words were never written"
            if name in want:
                assert torch.equal(v.view(torch.int32), want[name].view(torch.int32)), f"{name}: differs from the wrapper's result"


@gpu
@pytest.mark.parametrize("prec", ["fp32", "f16x3", "bf16"])
@pytest.mark.parametrize("K", [64, 512])
@pytest.mark.parametrize("M", [1, 17, 129, 257, 300])
def test_c_linear(M, K, prec):
    L = _lib.lib()
    for N in (64, 96, 130, 512):
        if prec == "bf16" and N % 8:
            continue
        A, W, b, R = _lin_operands(M, N, K)
        for epi, r in (("none", None), ("gelu", None), ("residual", R)):
            want = _E().op_linear(A, W, b, residual=r, epi=epi, precision=prec)
            o = _Outs()
            c = o.new((M, N), "C")
            _lib.check(L.d3d_op_linear(_p(_in(A)), _p(_in(W)), _p(_in(b)), _p(_in(r)), _p(c), M, N, K, {"none": 0, "gelu": 1, "residual": 2}[epi],
                                       _lib.PRECISIONS[prec], _st()))
            o.verify({"C": want})


ATTN_SMALL = [(2, 5, 17, 512, False), (2, 9, 17, 32, False), (2, 81, 3, 512, True), (1, 243, 2, 512, True), (2, 27, 17, 512, False),
              (2, 27, 17, 512, True)]


# every precision the hook accepts for the shape: the bf16 kernel takes head width 64 only
ATTN_C = [c + (p,) for c in ATTN_SMALL for p in ("fp32", "f16x3", "bf16") if p != "bf16" or c[3] // H == 64]


@gpu
@pytest.mark.parametrize("B,T,J,Dm,temporal,prec", ATTN_C)
def test_c_attention(B, T, J, Dm, temporal, prec):
    qkv = hashed(f"isoqkv{T}_{J}_{Dm}_{B}", (B * T * J, 3 * Dm), 21, 2.0).cuda()
    want = _E().op_attention(qkv, B, T, J, H, temporal, precision=prec)
    o = _Outs()
    out = o.new((B * T * J, Dm), "out")
    _lib.check(_lib.lib().d3d_op_attention(_p(_in(qkv)), _p(out), B, T, J, Dm, H, int(temporal), _lib.PRECISIONS[prec], 0, _st()))
    o.verify({"out": want})


@gpu
@pytest.mark.parametrize("rows,Dm", [(5, 32), (333, 512)])
def test_c_layernorm(rows, Dm):
    x = hashed("isolnx", (rows, Dm), 3, 3.0).cuda() + 0.7
    g, be = (1 + 0.1 * hashed("isolng", (Dm,), 4)).cuda(), (0.1 * hashed("isolnb", (Dm,), 5)).cuda()
    want = _E().op_layernorm(x, g, be, 1e-6)
    o = _Outs()
    out = o.new((rows, Dm), "out")
    _lib.check(_lib.lib().d3d_op_layernorm(_p(_in(x)), _p(_in(g)), _p(_in(be)), _p(out), rows, Dm, 1e-6, _st()))
    o.verify({"out": want})


@gpu
@pytest.mark.parametrize("rows", [1, 33, 4131])
def test_c_head(rows):
    eng = _head_engine()
    X = hashed(f"isohead{rows}", (rows, 512), 12, 1.7).cuda() + 0.3
    want = eng.head(X)
    o = _Outs()
    out = o.new((rows, 3), "x0")
    _lib.check(_lib.lib().d3d_op_head(eng._h, _p(_in(X)), _p(out), rows, _st()))
    o.verify({"x0": want})


def _rc_args(kw, N):
    pos, tv = kw["pos"], kw["tvec"]
    stride = 0 if tv.shape[0] == 1 else N
    return pos, int(kw["pos_div"]), int(pos.shape[0]), tv, stride, int(kw["rows_per_batch"])


@gpu
@pytest.mark.parametrize("with_stats", [False, True])
@pytest.mark.parametrize("M", [17, 300])
def test_c_linear_postnorm(M, with_stats):
    N, K = 512, 512
    A, W, b, R = _lin_operands(M, N, K)
    g, be = _gb(N)
    kw = _row_classes(M, N)
    wy, wst, _ = _E().op_linear_postnorm(A, W, b, R, g, be, 1e-6, with_stats=with_stats, **kw)
    pos, pos_div, pos_mod, tv, stride, rpb = _rc_args(kw, N)
    o = _Outs()
    y = o.new((M, N), "Y")
    st = o.new((M, 2), "stats") if with_stats else None
    ms = C.c_float(0.0)
    _lib.check(_lib.lib().d3d_op_linear_postnorm(_p(_in(A)), _p(_in(W)), _p(_in(b)), _p(_in(R)), _p(_in(g)), _p(_in(be)), 1e-6, _p(_in(pos)),
                                                 pos_div, pos_mod, _p(_in(tv)), stride, rpb, _p(y), _p(st), M, N, K, 1, C.byref(ms), _st()))
    o.verify({"Y": wy, "stats": wst} if with_stats else {"Y": wy})


@gpu
@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("op", ["postnorm", "postnorm_stats", "residual", "gelu"])
def test_c_splitk(op, S):
    E, L = _E(), _lib.lib()
    M, K = 130, 512
    N = 1024 if op == "gelu" else 512
    A, W, b, R = _lin_operands(M, N, K)
    o = _Outs()
    y = o.new((M, N), "Y")
    part = o.new((S, M, N), "partials")
    ms = C.c_float(0.0)
    if op == "gelu":
        g, be = _gb(K)
        want = {"Y": E.op_linear_splitk_gelu(A, W, b, g, be, 1e-6, S=S)[0]}
        _lib.check(L.d3d_op_linear_splitk_gelu(_p(_in(A)), _p(_in(W)), _p(_in(b)), _p(_in(g)), _p(_in(be)), 1e-6, _p(y), M, N, K, S, _p(part),
                                               1, C.byref(ms), _st()))
    elif op == "residual":
        wy, wst, _ = E.op_linear_splitk_residual(A, W, b, R, S=S, with_stats=True)
        want = {"Y": wy, "stats": wst}
        st = o.new((M, N // 64, 2), "stats")
        _lib.check(L.d3d_op_linear_splitk_residual(_p(_in(A)), _p(_in(W)), _p(_in(b)), _p(_in(R)), _p(y), _p(st), M, N, K, S, _p(part), 1,
                                                   C.byref(ms), _st()))
    else:
        g, be = _gb(N)
        kw = _row_classes(M, N)
        ws = op == "postnorm_stats"
        wy, wst, _ = E.op_linear_splitk_postnorm(A, W, b, R, g, be, 1e-6, S=S, with_stats=ws, **kw)
        want = {"Y": wy, "stats": wst} if ws else {"Y": wy}
        st = o.new((M, 2), "stats") if ws else None
        pos, pos_div, pos_mod, tv, stride, rpb = _rc_args(kw, N)
        _lib.check(L.d3d_op_linear_splitk_postnorm(_p(_in(A)), _p(_in(W)), _p(_in(b)), _p(_in(R)), _p(_in(g)), _p(_in(be)), 1e-6, _p(_in(pos)),
                                                   pos_div, pos_mod, _p(_in(tv)), stride, rpb, _p(y), _p(st), M, N, K, S, _p(part), 1,
                                                   C.byref(ms), _st()))
    o.verify(want)


@gpu
@pytest.mark.parametrize("B,T,J,temporal", [(1, 31, 17, False), (2, 27, 17, True)])
def test_c_qkv_attn_bf16(B, T, J, temporal):
    from diff3dhpe_amd.synth import synth_state_dict
    sd = synth_state_dict(cfg_full(27), 11)
    kw = [k for k in sd if k.endswith("attn.qkv.weight")][2]
    W, b = torch.from_numpy(sd[kw]).cuda(), torch.from_numpy(sd[kw.replace("weight", "bias")]).cuda()
    A = hashed(f"isofa{T}", (B * T * J, D), 31, 1.0).cuda()
    groups, N, stride = (B * J, T, J) if temporal else (B * T, J, 1)
    want = _E().op_qkv_attn_bf16(A, W, b, groups, N, stride, H, temporal)
    o = _Outs()
    out = o.new((B * T * J, D), "out")
    _lib.check(_lib.lib().d3d_op_qkv_attn_bf16(_p(_in(A)), _p(_in(W)), _p(_in(b)), groups, N, stride, D, H, int(temporal), _p(out), _st()))
    o.verify({"out": want})


ENGINE_C = [("fp32", 27, 2, ()), ("f16x3", 27, 2, ()), ("bf16", 27, 2, ()), ("f16x3", 243, 1, ()),
            ("f16x3", 27, 2, (("latency_mode", 1), ("proj_split", 2), ("fc1_split", 2))),
            ("f16x3", 27, 2, (("latency_mode", 1), ("proj_split", 4), ("fc1_split", 4)))]


@gpu
@pytest.mark.parametrize("prec,T,B,opts", ENGINE_C, ids=[f"{p}-T{T}-B{B}" + ("-latency%d" % o[1][1] if o else "") for p, T, B, o in ENGINE_C])
def test_c_engine_calls(prec, T, B, opts):
    """d3d_denoise, d3d_ddim_sample without and with trajectory: out / rev / x0s and a workspace of exactly d3d_workspace_bytes(B) bytes in
    bands (the workspace's interior is scratch: only its bands are checked)."""
    L = _lib.lib()
    cfg = cfg_full(T)
    eng = _engine(cfg, prec, opts)
    inp = inputs(B, T, 311)
    x2d, y = inp["x2d"].cuda(), inp["noise"].cuda()
    t = torch.tensor([(431 * i + 77) % 1000 for i in range(B)], dtype=torch.float32, device="cuda")
    S, J = 3, cfg.num_joints
    want_den = eng.denoise(x2d, y, t).clone()
    want_y0 = eng.ddim_sample(x2d, y).clone()
    wy, wrev, wx0 = (r.clone() for r in eng.ddim_sample(x2d, y, trajectory=True))
    if opts:
        assert (eng.info("proj_split_last"), eng.info("fc1_split_last")) == (opts[1][1], opts[2][1])
    assert torch.equal(wy, want_y0)
    nbytes = L.d3d_workspace_bytes(eng._h, B)
    ws, ws_check = banded((nbytes,), dtype=torch.uint8)
    bx, by, bt = _in(x2d), _in(y), _in(t)
    with eng.lock:
        o = _Outs()
        out = o.new((B, T, J, 3), "out")
        _lib.check(L.d3d_denoise(eng._h, _p(bx), _p(by), T, _p(bt), B, _p(out), B, _p(ws), nbytes, _st()))
        o.verify({"out": want_den})
        ws_check()
        o = _Outs()
        out = o.new((B, T, J, 3), "out")
        _lib.check(L.d3d_ddim_sample(eng._h, _p(bx), _p(by), None, _p(out), None, None, B, _p(ws), nbytes, _st()))
        o.verify({"out": want_y0})
        ws_check()
        o = _Outs()
        out, rev, x0s = o.new((B, T, J, 3), "out"), o.new((B, T, J, 3, S), "rev"), o.new((B, T, J, 3, S), "x0s")
        _lib.check(L.d3d_ddim_sample(eng._h, _p(bx), _p(by), None, _p(out), _p(rev), _p(x0s), B, _p(ws), nbytes, _st()))
        o.verify({"out": wy, "rev": wrev, "x0s": wx0})
        ws_check()
