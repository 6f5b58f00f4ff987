"""Exact fp32 attention for heads of 32 columns on the MI355X ("attn_f32_h32", kernels_attn_f32_h32.hip): embed_dim 256 with the runner's
8 heads on an FP32 engine -- the exact mode, and the engine a precision-"auto" model falls back to.
  * op level against fp64 math at every group length: temporal N = 1 .. 256 per key-tile class, spatial 15 / 16 / 17 joints at 1, 3, 4 and
    13 frames (8, 24, 32, 104 units: a partly filled workgroup, a partly filled wave, a last workgroup with surplus waves); finite, the
    same bits twice, not the generic kernel's bits throughout a class;
  * narrow and odd head counts; sharp softmax; a NaN batch element does not reach its neighbour; refusals;
  * engine level against the fp64 oracle with the option on and off, invariances, proof of the path through info("attn_f32_h32_last"),
    the fallback engine of precision "auto".

The op-level bound is that of tests/test_gpu_group_lengths.py: err(N) <= max(5e-6, 2 e32(N)), where e32(N) is the error of the same
formula in plain fp32 torch on the CPU on the same input.

Measured maxima (MI355X), max-abs against fp64 (the N of the maximum in brackets; e32 there):

  key tiles         1             2             3             4              5              6              7              8
  temporal     9.16e-7 (21)  9.90e-7 (47)  1.22e-6 (74)  1.38e-6 (127)  1.28e-6 (137)  1.25e-6 (180)  1.67e-6 (215)  1.25e-6 (250)
    e32 there  1.27e-6       1.51e-6       1.59e-6       2.18e-6        2.46e-6        3.17e-6        2.27e-6        2.18e-6
  spatial      15 joints 7.45e-7, 16 joints 6.98e-7, 17 joints 9.38e-7 (13 frames each; e32 8.7e-7, 9.4e-7, 8.8e-7)
  narrow / odd head counts: 6.47e-7, 6.73e-7, 5.88e-7; sharp softmax: spatial 6.6e-5 (generic 6.6e-5), temporal 1.32e-4 (generic 1.05e-4)
  engine against the oracle, option on / off: T = 27 1.01e-6 / 1.23e-6, T = 243 2.82e-6 / 3.06e-6
"""
import warnings

import pytest
import torch

import group_lengths as gl
from helpers import hashed, inputs, maxabs, attn_ref, torch_sd, build_net, product_with_engine, xy
from diff3dhpe_amd._lib import D3DError
from diff3dhpe_amd.spec import DenoiserConfig

pytestmark = pytest.mark.gpu
GATE = 1e-4
FLOOR = 5e-6          # test_attention_core's bound for hashed qkv at scale 2.0
DEPTH = 1
KEY, LAST = "attn_f32_h32", "attn_f32_h32_last"
B, J, H, D = 2, 3, 8, 256          # the temporal sweep: stride J = 3
SPATIAL_FRAMES = (1, 3, 4, 13)


def _eng():
    from diff3dhpe_amd import engine
    return engine


def _bound(qkv_cpu, Bn, T, Jn, Hn, temporal):
    """(fp64 reference, max(5e-6, 2 e32), e32) of one problem, on the CPU."""
    ref = attn_ref(qkv_cpu, Bn, T, Jn, Hn, temporal)
    e32 = maxabs(attn_ref(qkv_cpu, Bn, T, Jn, Hn, temporal, torch.float32), ref)
    return ref, max(FLOOR, 2 * e32), e32


# ------------------------------------------------------------------------------------------------ 1. every group length against fp64
_BASE = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_base():
    yield
    _BASE.clear()


def _base(name, rows):
    """(cpu, device) hashed qkv rows at scale 2.0, made once; a case takes the first rows it needs."""
    if name not in _BASE:
        x = hashed(name, (rows, 3 * D), 21, 2.0)
        _BASE[name] = (x, x.cuda())
    return _BASE[name]


def _sweep(what, cases, run, generic):
    """cases: [(label, qkv on the device, reference, bound, e32)].  Every failing case is reported at once; the worst error is printed."""
    fails, worst, differs = [], (-1.0, None, ""), False
    for label, q, ref, bound, e32 in cases:
        out = run(q)
        err = maxabs(out, ref)
        if not err <= worst[0]:
            worst = (err, label, f" (e32 {e32:.3e}, bound {bound:.3e})")
        if not torch.isfinite(out).all():
            fails.append(f"{label}: the output is not finite")
        if not err <= bound:
            fails.append(f"{label}: err {err:.3e} > {bound:.3e} (e32 {e32:.3e})")
        if not torch.equal(run(q), out):
            fails.append(f"{label}: a second call gives other bits")
        if not torch.equal(generic(q), out):
            differs = True
    print(f"attn_f32_h32 [{what}]: max err {worst[0]:.3e} at {worst[1]}{worst[2]}")
    if not differs:
        fails.append("every case gives the generic kernel's bits: the new kernel did not run")
    assert not fails, f"{what}:\n" + "\n".join(fails)


@pytest.mark.parametrize("c", range(1, 9))
def test_temporal_kernel_matches_fp64_at_every_length(c):
    E = _eng()
    cpu, dev = _base("f32h32_tp", B * gl.RESIDENT_MAX * J)
    lengths = [N for N in range(1, gl.RESIDENT_MAX + 1) if gl.nkt(N) == c]
    assert len(lengths) == 32
    cases = []
    for N in lengths:
        rows = B * N * J
        ref, bound, e32 = _bound(cpu[:rows], B, N, J, H, True)
        cases.append((f"N = {N}", (dev[:rows], N), ref, bound, e32))
    _sweep(f"temporal, {c} key tiles", cases, lambda a: E.op_attention_f32_h32(a[0], B, a[1], J, H, True),
           lambda a: E.op_attention(a[0], B, a[1], J, H, True, force_generic=True))


@pytest.mark.parametrize("Jn", [15, 16, 17])
def test_spatial_kernel_matches_fp64(Jn):
    """One batch element of 1, 3, 4 and 13 frames x 8 heads = 8, 24, 32, 104 units; a workgroup takes 16 units (12 at 17 joints), a wave 4
    (3): less than one workgroup, a partly filled wave, whole workgroups, and a last workgroup with surplus waves."""
    E = _eng()
    cpu, dev = _base(f"f32h32_sp{Jn}", max(SPATIAL_FRAMES) * Jn)
    cases = []
    for T in SPATIAL_FRAMES:
        rows = T * Jn
        ref, bound, e32 = _bound(cpu[:rows], 1, T, Jn, H, False)
        cases.append((f"{T} frames", (dev[:rows], T), ref, bound, e32))
    _sweep(f"spatial, {Jn} joints", cases, lambda a: E.op_attention_f32_h32(a[0], 1, a[1], Jn, H, False),
           lambda a: E.op_attention(a[0], 1, a[1], Jn, H, False, force_generic=True))


# ------------------------------------------------------------------------------------------------ 2. narrow and odd head counts
@pytest.mark.parametrize("Bn,T,Jn,Dn,Hn,temporal", [(1, 33, 2, 64, 2, True), (2, 27, 3, 96, 3, True), (2, 5, 16, 64, 2, False)])
def test_narrow_and_odd_head_counts(Bn, T, Jn, Dn, Hn, temporal):
    E = _eng()
    cpu = hashed(f"qkv{T}_{Jn}_{Dn}", (Bn * T * Jn, 3 * Dn), 21, 2.0)
    ref, bound, e32 = _bound(cpu, Bn, T, Jn, Hn, temporal)
    got = E.op_attention_f32_h32(cpu.cuda(), Bn, T, Jn, Hn, temporal)
    err = maxabs(got, ref)
    print(f"attn_f32_h32 B={Bn} T={T} J={Jn} D={Dn} H={Hn} temporal={int(temporal)}: max-abs {err:.3e} (e32 {e32:.3e}, bound {bound:.3e})")
    assert torch.isfinite(got).all()
    assert err <= bound


# ------------------------------------------------------------------------------------------------ 3. sharp softmax
@pytest.mark.parametrize("Bn,T,Jn,temporal", [(2, 7, 17, False), (1, 243, 3, True)])
def test_sharp_softmax(Bn, T, Jn, temporal):
    """Logits up to ~100 (near one-hot rows): the bound of tests/test_gpu_ops.py::test_attention_fast_kernels_agree_with_generic_on_sharp_softmax."""
    E = _eng()
    qkv = hashed(f"sharp{T}", (Bn * T * Jn, 3 * D), 22, 9.0).cuda()
    ref = attn_ref(qkv, Bn, T, Jn, H, temporal).cpu()
    a = E.op_attention_f32_h32(qkv, Bn, T, Jn, H, temporal)
    b = E.op_attention(qkv, Bn, T, Jn, H, temporal, force_generic=True)
    print(f"attn_f32_h32 sharp T={T} J={Jn}: new {maxabs(a, ref):.3e} generic {maxabs(b, ref):.3e} apart {maxabs(a, b.cpu()):.3e}")
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert maxabs(a, ref) < 2e-3 and maxabs(b, ref) < 2e-3
    assert maxabs(a, b.cpu()) < 2e-3


# ------------------------------------------------------------------------------------------------ 4. isolation
@pytest.mark.parametrize("T,Jn,temporal", [(243, 2, True), (5, 17, False)])
def test_a_nan_batch_element_does_not_reach_its_neighbour(T, Jn, temporal):
    E = _eng()
    Bn = 2
    qkv = hashed(f"isoqkv{T}_{Jn}_{D}_{Bn}", (Bn * T * Jn, 3 * D), 21, 2.0).cuda()
    bad = qkv.clone()
    bad[T * Jn:] = float("nan")
    alone = E.op_attention_f32_h32(qkv[:T * Jn].contiguous(), 1, T, Jn, H, temporal)
    both = E.op_attention_f32_h32(bad, Bn, T, Jn, H, temporal)
    assert torch.isfinite(both[:T * Jn]).all()
    assert torch.equal(both[:T * Jn], alone)


# ------------------------------------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("T,Jn,Dn,Hn,temporal", [(27, 2, 512, 8, True), (27, 17, 512, 8, False), (257, 2, 256, 8, True), (2, 21, 256, 8, False)])
def test_refuses_other_widths_long_windows_and_other_joint_counts(T, Jn, Dn, Hn, temporal):
    qkv = torch.zeros((T * Jn, 3 * Dn), device="cuda")
    with pytest.raises(D3DError, match="head_dim 32"):
        _eng().op_attention_f32_h32(qkv, 1, T, Jn, Hn, temporal)


# ------------------------------------------------------------------------------------------------ 6. - 9. engine level
def _cfg(T, Dn=256, Jn=17):
    return DenoiserConfig(num_frame=T, num_joints=Jn, embed_dim=Dn, depth=DEPTH, num_heads=8)


def _sd(cfg, seed=11):   # this module's weights: seed 11 of the trained-like family
    return torch_sd(cfg, seed, family="trainedlike")


def _net(cfg, seed=11, prec="fp32"):
    return build_net(cfg, seed, prec, family="trainedlike")


def _product(cfg, seed=11, prec="fp32", sampling=2):   # this module's defaults; the weights of _sd
    return product_with_engine(cfg, seed, prec, sampling, family="trainedlike")


def _sample(eng, x2d, nz):   # reads this feature's proof-of-path key, LAST
    out = eng.ddim_sample(x2d, nz).clone()
    return out, eng.info(LAST)


@pytest.mark.parametrize("T", [27, 243])
def test_forward_denoise_against_the_oracle_with_the_option_on_and_off(T):
    """forward_denoise of an FP32 engine at B = 2, trained-like weights, depth 1, per-row t, against oracle/d3d_oracle.py in fp64: the
    kernels for heads of 32 columns and the generic kernel both inside the project's 1e-4 gate."""
    from oracle import d3d_oracle as orc
    cfg = _cfg(T)
    net, _, eng = _product(cfg)
    sd = _sd(cfg)
    inp = inputs(2, T, 500)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1)
    t = torch.tensor([905, 17], dtype=torch.long)
    ref32 = orc.forward_denoise(sd, xcat, t, depth=DEPTH)
    torch.set_default_dtype(torch.float64)      # (the oracle's sinusoid and identity follow the default dtype)
    try:
        ref64 = orc.forward_denoise({k: v.double() for k, v in sd.items()}, xcat.double(), t, depth=DEPTH)
    finally:
        torch.set_default_dtype(torch.float32)
    assert ref64.dtype == torch.float64
    floor = (ref32.double() - ref64).abs().max().item()
    default = eng.info(KEY)
    err = {}
    try:
        for opt in (1, 0):
            eng.set_option(KEY, opt)
            out = net.forward_denoise(xcat.cuda(), t.cuda())
            assert eng.info(LAST) == (3 if opt else 0)
            err[opt] = (out.cpu().double() - ref64).abs().max().item()
    finally:
        eng.set_option(KEY, default)
    print(f"attn_f32_h32 T={T} B=2: err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}")
    assert err[1] <= GATE and err[0] <= GATE


def test_rows_do_not_depend_on_batch_streams_workspace_contents_or_graph_replay():
    T, Bn = 27, 3
    _, _, eng = _product(_cfg(T))
    eng.set_option(KEY, 1)
    x2d, nz = xy(Bn, T, 80)
    eng.set_option("streams", 2)
    whole, last = _sample(eng, x2d, nz)
    assert last == 3 and torch.isfinite(whole).all()
    for b in range(Bn):
        one, last = _sample(eng, x2d[b:b + 1].contiguous(), nz[b:b + 1].contiguous())
        assert last == 3 and torch.equal(one, whole[b:b + 1])
    eng.set_option("streams", 1)
    assert torch.equal(_sample(eng, x2d, nz)[0], whole)
    eng.set_option("streams", 2)
    eng._workspace(Bn).view(torch.float32).fill_(float("nan"))
    assert torch.equal(_sample(eng, x2d, nz)[0], whole)
    eng.set_graph_mode(True)
    try:
        first, l1 = _sample(eng, x2d, nz)          # eager warm-up pass + capture + replay
        again = eng.ddim_sample(x2d, nz).clone()   # replay of the cached graph
        assert eng.info("graphs_cached") >= 1
    finally:
        eng.set_graph_mode(False)
    assert l1 == 3
    assert torch.equal(first, whole) and torch.equal(again, whole)


@pytest.mark.parametrize("T,Jn,want", [(27, 21, 2), (300, 17, 1)])
def test_each_block_type_takes_its_kernel_where_its_group_length_fits(T, Jn, want):
    """21 joints: the spatial blocks stay on k_attn_generic; 300 frames: the temporal blocks do."""
    _, _, eng = _product(_cfg(T, Jn=Jn))
    eng.set_option(KEY, 1)
    assert eng.info(LAST) == 0                     # before any forward
    out, last = _sample(eng, *xy(1, T, 83, Jn))
    assert last == want and torch.isfinite(out).all()


def test_engines_with_heads_of_64_columns_ignore_the_option():
    T = 27
    _, _, eng = _product(_cfg(T, Dn=512))
    x2d, nz = xy(2, T, 82)
    default = eng.info(KEY)
    res = {}
    try:
        for opt in (1, 0):
            eng.set_option(KEY, opt)
            res[opt] = _sample(eng, x2d, nz)
    finally:
        eng.set_option(KEY, default)
    assert (res[1][1], res[0][1]) == (0, 0)
    assert torch.isfinite(res[1][0]).all() and torch.equal(res[1][0], res[0][0])


def test_f16x3_engines_are_left_alone():
    """Neither flow of an F16X3 engine at embed_dim 256 -- the folded one on the F16X3 kernel of this width, the plain one "attn_h32" = 0
    selects (which calls the same attention dispatch with the generic kernel) -- takes the fp32 kernels, and neither changes a bit."""
    T = 27
    _, _, e3 = _product(_cfg(T), prec="f16x3")
    x2d, nz = xy(1, T, 83)
    default, flow_default = e3.info(KEY), e3.info("attn_h32")
    assert e3.info(LAST) == 0
    try:
        for flow in (1, 0):
            e3.set_option("attn_h32", flow)
            res = {}
            for opt in (1, 0):
                e3.set_option(KEY, opt)
                res[opt] = e3.ddim_sample(x2d, nz).clone()
                assert e3.info("attn_h32_last") == flow and e3.info(LAST) == 0
            assert torch.isfinite(res[1]).all() and torch.equal(res[1], res[0])
    finally:
        e3.set_option("attn_h32", flow_default)
        e3.set_option(KEY, default)


def test_the_auto_fallback_engine_runs_the_kernels():
    """precision "auto" at T = 27, embed_dim 256: an input scaled past the plane range raises the F16X3 guard, the call is repeated on the
    exact-fp32 engine -- ONE warning, the fp32 model's result bit for bit, and that engine's blocks on the kernels for heads of 32 columns."""
    T, Bn = 27, 2
    cfg = _cfg(T)
    net = _net(cfg, prec="auto").cuda()
    net32 = _net(cfg, prec="fp32").cuda()
    dev = torch.device("cuda", torch.cuda.current_device())
    net.engine_for(dev, True).set_option(KEY, 1)       # (whatever the default is)
    net32.engine_for(dev).set_option(KEY, 1)
    x2d, nz = xy(Bn, T, 81)
    big = torch.cat([x2d * 1.0e6, nz], dim=-1)
    t = torch.arange(Bn, device="cuda") * 300 + 11
    want = net32.forward_denoise(big, t).clone()
    with warnings.catch_warnings(record=True) as wlog:
        warnings.simplefilter("always")
        got = net.forward_denoise(big, t).clone()
    ours = [w for w in wlog if issubclass(w.category, RuntimeWarning)]
    assert len(ours) == 1 and "range guard fired" in str(ours[0].message), [str(w.message) for w in wlog]
    assert torch.equal(got, want)
    assert net._on_fallback()
    assert net.engine_for(dev, True).info(LAST) == 3
    assert net32.engine_for(dev).info(LAST) == 3
