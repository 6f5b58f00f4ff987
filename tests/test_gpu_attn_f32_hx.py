"""Exact fp32 attention for heads of 48 and 96 columns on the MI355X ("attn_f32_hx", kernels_attn_f32_hx.hip): embed_dim 384 / 768 with
the runner's 8 heads on an FP32 engine -- the exact mode, and the engine a precision-"auto" model falls back to.  Every test runs at both
widths.
  * op level against fp64 math: the resident kernel at every group length N = 1 .. 256 (width 48) / 192 (width 96) per key-tile class
    (finite, the same bits twice, not the generic kernel's bits throughout a class), spatial groups of 15 / 16 / 17 / 21 / 33 joints;
  * the key-streaming kernel on both sides of the chunk boundary (256 / 192 frames) and of the query-block boundary (256), and bit for
    bit the resident kernel at every T it takes;
  * head isolation, the case particular to these widths: a head filled with NaN leaves its neighbours' bits alone (at width 48 the second
    accumulator tile spans the next head's first 16 columns); batch isolation; sharp softmax; refusals;
  * engine level against the fp64 oracle with the option on and off, invariances, proof of the path through info("attn_f32_hx_last"),
    each block type deciding alone, the other widths and precisions left alone, the fallback engine of precision "auto".

The op-level bound is that of tests/test_gpu_attn_f32_h128.py: err <= max(5e-6, 2 e32), where e32 is the error of the same formula in
plain fp32 torch on the CPU on the same input.  The sweeps run H = 2 heads (D = 96 / 192), B = 2, J = 3.

Measured maxima (MI355X), max-abs against fp64 (e32 on the same input in brackets; the bound was 5e-6 .. 6.4e-6 everywhere):

  resident, width 48, key tiles 1 .. 8: 1.06e-6 (N = 24; 8.0e-7), 1.08e-6 (37; 1.31e-6), 8.4e-7 (73; 1.55e-6), 1.49e-6 (113; 1.90e-6),
    1.22e-6 (140; 2.45e-6), 1.08e-6 (165; 2.42e-6), 1.11e-6 (198; 1.98e-6), 9.7e-7 (246; 2.07e-6)
  resident, width 96, key tiles 1 .. 6: 1.25e-6 (N = 14; 1.48e-6), 1.48e-6 (49; 1.51e-6), 1.49e-6 (80; 1.93e-6), 1.50e-6 (106; 2.07e-6),
    1.57e-6 (151; 2.62e-6), 1.47e-6 (161; 2.87e-6)
  spatial, 1 / 3 / 13 frames, width 48 / 96: 15 joints 8.1e-7 / 1.38e-6, 16 joints 7.9e-7 / 1.31e-6, 17 joints 7.2e-7 / 1.88e-6 (e32
    9.2e-7 .. 1.38e-6); 21 joints 7.0e-7 / 1.00e-6, 33 joints 4.8e-7 / 6.3e-7, (2, 5, 17, D, 8) 7.9e-7 / 1.46e-6; resident
    (2, 81, 17, D, 8) 1.13e-6 / 1.41e-6 (2.0e-6 / 2.3e-6)
  streaming sweep, width 48 1.10e-6 at T = 513 (2.82e-6), width 96 1.54e-6 at T = 33 (1.45e-6); (3, 243, 17, D, 8) 1.86e-6 (3.04e-6) /
    1.73e-6 (3.19e-6)
  sharp softmax, new / generic / apart: spatial 6.1e-5 / 7.2e-5 / 9.2e-5 (width 48), 1.52e-4 / 1.16e-4 / 1.51e-4 (96); resident T = 100
    9.0e-5 / 8.7e-5 / 9.4e-5, 1.79e-4 / 1.23e-4 / 1.81e-4; streaming T = 300 1.53e-4 / 1.49e-4 / 1.40e-4, 2.32e-4 / 2.12e-4 / 2.50e-4
  engine against the oracle, option on / off (oracle fp32 floor): D = 384 T = 27 2.96e-6 / 3.35e-6 (3.20e-6), T = 300 3.86e-6 / 4.51e-6
    (4.45e-6); D = 768 T = 27 3.29e-6 / 3.23e-6 (3.32e-6), T = 243 4.98e-6 / 4.98e-6 (3.85e-6)
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
KEY, LAST = "attn_f32_hx", "attn_f32_hx_last"
WIDTHS = [48, 96]
RESIDENT_MAX = {48: 256, 96: 192}  # the longest group whose keys stay in LDS (8 / 6 key tiles); also the streaming kernel's chunk
B, J, H = 2, 3, 2                  # the sweeps: stride J = 3, two heads (D = 2 DH)
# the "*_last" keys of the other attention families: none of them may move on an engine that takes these kernels
OTHER_LAST = ("long_temporal_last", "attn_h32_last", "long_temporal_h32_last", "attn_h128_last", "attn_hx_last", "long_temporal_f32_last",
              "attn_f32_h32_last", "long_temporal_f32_h32_last", "attn_f32_h128_last")


def _eng():
    from diff3dhpe_amd import engine
    return engine


def _bound(qkv_cpu, Bn, T, Jn, Hn, temporal):
    """(fp64 reference, max(5e-6, 2 e32), e32) of one problem, on the CPU."""
    ref = attn_ref(qkv_cpu, Bn, T, Jn, Hn, temporal)
    e32 = maxabs(attn_ref(qkv_cpu, Bn, T, Jn, Hn, temporal, torch.float32), ref)
    return ref, max(FLOOR, 2 * e32), e32


_BASE = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_base():
    yield
    _BASE.clear()


def _base(name, rows, Dn, seed=21, scale=2.0):
    """(cpu, device) hashed qkv rows, made once; a case takes the first rows it needs."""
    key = (name, Dn)
    if key not in _BASE:
        x = hashed(f"{name}_{Dn}", (rows, 3 * Dn), seed, scale)
        _BASE[key] = (x, x.cuda())
    assert _BASE[key][0].shape[0] >= rows
    return _BASE[key]


def _sweep(what, cases, run, generic):
    """cases: [(label, argument of run / generic, reference, bound, e32)].  Every failing case is reported at once; the worst error is
    printed."""
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
    print(f"attn_f32_hx [{what}]: max err {worst[0]:.3e} at {worst[1]}{worst[2]}")
    if not differs:
        fails.append("every case gives the generic kernel's bits: the new kernel did not run")
    assert not fails, f"{what}:\n" + "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 1. resident, every N
CLASSES = [(DH, c) for DH in WIDTHS for c in range(1, RESIDENT_MAX[DH] // 32 + 1)]


@pytest.mark.parametrize("DH,c", CLASSES, ids=[f"dh{d}_tiles{c}" for d, c in CLASSES])
def test_resident_kernel_matches_fp64_at_every_length(DH, c):
    E = _eng()
    Dn, NMAX = H * DH, RESIDENT_MAX[DH]
    cpu, dev = _base("f32hx_tp", B * 256 * J, Dn)
    lengths = [N for N in range(1, NMAX + 1) if gl.nkt(N) == c]
    assert len(lengths) == 32
    cases = []
    for N in lengths:
        rows = B * N * J
        ref, bound, e32 = _bound(cpu[:rows], B, N, J, H, True)
        cases.append((f"N = {N}", (dev[:rows], N), ref, bound, e32))
    _sweep(f"dh {DH} temporal resident, {c} key tiles", cases, lambda a: E.op_attention_f32_hx(a[0], B, a[1], J, H, True),
           lambda a: E.op_attention(a[0], B, a[1], J, H, True, force_generic=True))


# ------------------------------------------------------------------------------------------------ 2. spatial
SPATIAL_FRAMES = (1, 3, 13)


@pytest.mark.parametrize("DH", WIDTHS)
@pytest.mark.parametrize("Jn", [15, 16, 17])
def test_spatial_groups_match_fp64(Jn, DH):
    """One batch element of 1, 3 and 13 frames: a spatial call is (B T, J, 1), one workgroup of one wave per (frame, head)."""
    E = _eng()
    Dn = H * DH
    cpu, dev = _base(f"f32hx_sp{Jn}", max(SPATIAL_FRAMES) * Jn, Dn)
    cases = []
    for T in SPATIAL_FRAMES:
        rows = T * Jn
        ref, bound, e32 = _bound(cpu[:rows], 1, T, Jn, H, False)
        cases.append((f"{T} frames", (dev[:rows], T), ref, bound, e32))
    _sweep(f"dh {DH} spatial, {Jn} joints", cases, lambda a: E.op_attention_f32_hx(a[0], 1, a[1], Jn, H, False),
           lambda a: E.op_attention(a[0], 1, a[1], Jn, H, False, force_generic=True))


def _one(E, what, Bn, T, Jn, Dn, Hn, temporal, run=None):
    """One shape against fp64 under the bound of this file; the same bits twice.  Returns the output."""
    cpu = hashed(f"qkv{T}_{Jn}_{Dn}", (Bn * T * Jn, 3 * Dn), 21, 2.0)
    ref, bound, e32 = _bound(cpu, Bn, T, Jn, Hn, temporal)
    run = run or (lambda q: E.op_attention_f32_hx(q, Bn, T, Jn, Hn, temporal))
    dev = cpu.cuda()
    got = run(dev)
    err = maxabs(got, ref)
    print(f"attn_f32_hx [{what}] B={Bn} T={T} J={Jn} D={Dn} H={Hn} temporal={int(temporal)}: max-abs {err:.3e} (e32 {e32:.3e}, "
          f"bound {bound:.3e})")
    assert torch.isfinite(got).all()
    assert err <= bound
    assert torch.equal(run(dev), got)
    return got


@pytest.mark.parametrize("DH", WIDTHS)
@pytest.mark.parametrize("Bn,T,Jn,Hn", [(1, 2, 21, 2), (1, 1, 33, 1), (2, 5, 17, 8)], ids=["21joints", "33joints", "8heads"])
def test_spatial_other_joint_counts(Bn, T, Jn, Hn, DH):
    """21 joints (no other fp32 spatial kernel takes them); 33 joints: two key tiles, two waves, in a spatial call; the runner's 8 heads."""
    _one(_eng(), "spatial", Bn, T, Jn, Hn * DH, Hn, False)


@pytest.mark.parametrize("DH", WIDTHS)
def test_resident_kernel_with_eight_heads(DH):
    """embed_dim 384 / 768 as the engines run it: 8 heads, 17 joints, three key tiles."""
    _one(_eng(), "resident", 2, 81, 17, 8 * DH, 8, True)


# ------------------------------------------------------------------------------------------------ 3. streaming
def _stream_lengths(DH):
    """T = 1 and both sides of the key-tile boundary, of the chunk boundary (the resident maximum), of the query-block boundary (256);
    300 (two query blocks of 160), 513 (three of 192; three / four chunks)."""
    R = RESIDENT_MAX[DH]
    return sorted({1, 31, 32, 33, R - 1, R, R + 1, 255, 256, 257, 300, 513})


@pytest.mark.parametrize("DH", WIDTHS)
def test_streaming_kernel_matches_fp64(DH):
    E = _eng()
    Dn = H * DH
    cpu, dev = _base("f32hx_long", B * 513 * J, Dn)
    cases = []
    for T in _stream_lengths(DH):
        rows = B * T * J
        ref, bound, e32 = _bound(cpu[:rows], B, T, J, H, True)
        cases.append((f"T = {T}", (dev[:rows], T), ref, bound, e32))
    _sweep(f"dh {DH} streaming", cases, lambda a: E.op_attention_long_f32_hx(a[0], B, a[1], J, H),
           lambda a: E.op_attention(a[0], B, a[1], J, H, True, force_generic=True))


@pytest.mark.parametrize("DH", WIDTHS)
def test_streaming_kernel_at_the_runner_shape(DH):
    E = _eng()
    _one(E, "streaming", 3, 243, 17, 8 * DH, 8, True, run=lambda q: E.op_attention_long_f32_hx(q, 3, 243, 17, 8))


# ------------------------------------------------------------------------------------------------ 4. bit identity
@pytest.mark.parametrize("DH", WIDTHS)
@pytest.mark.parametrize("name,seed,scale", [("f32hx_bits", 21, 2.0), ("f32hx_sharp", 22, 9.0)], ids=["scale2", "sharp"])
def test_streaming_kernel_is_bit_identical_to_the_resident_one(name, seed, scale, DH):
    """Every T = 1 .. the resident maximum, so every wave count of the resident kernel and every pad-key count."""
    E = _eng()
    NMAX = RESIDENT_MAX[DH]
    _, dev = _base(name, B * 256 * J, H * DH, seed=seed, scale=scale)
    differ = []
    for T in range(1, NMAX + 1):
        q = dev[:B * T * J]
        a = E.op_attention_f32_hx(q, B, T, J, H, True)
        if not torch.equal(E.op_attention_long_f32_hx(q, B, T, J, H), a):
            differ.append(T)
        assert torch.isfinite(a).all(), T
    assert not differ, f"other bits at T = {differ}"


# ------------------------------------------------------------------------------------------------ 5. isolation
FORMS = [("resident", 2, 40, 3, True), ("spatial", 2, 5, 17, False), ("streaming", 1, 300, 2, True)]


def _run_form(E, form, q, Bn, T, Jn, Hn):
    if form == "streaming":
        return E.op_attention_long_f32_hx(q, Bn, T, Jn, Hn)
    return E.op_attention_f32_hx(q, Bn, T, Jn, Hn, form == "resident")


@pytest.mark.parametrize("DH", WIDTHS)
@pytest.mark.parametrize("Hn,bad", [(3, 1), (8, 3)], ids=["3heads", "8heads"])
@pytest.mark.parametrize("form,Bn,T,Jn,temporal", FORMS, ids=[f[0] for f in FORMS])
def test_a_nan_head_does_not_reach_its_neighbours(form, Bn, T, Jn, temporal, Hn, bad, DH):
    """q, k and v of one middle head are NaN in every token.  The heads on either side must be finite and bit-equal to the run on clean
    input: no accumulator tile, staging slot or store of a head may touch the next head's columns."""
    E = _eng()
    Dn = Hn * DH
    qkv = hashed(f"headiso{T}_{Jn}_{Dn}", (Bn * T * Jn, 3 * Dn), 21, 2.0).cuda()
    poisoned = qkv.clone()
    for third in range(3):
        poisoned[:, third * Dn + bad * DH: third * Dn + (bad + 1) * DH] = float("nan")
    clean = _run_form(E, form, qkv, Bn, T, Jn, Hn)
    got = _run_form(E, form, poisoned, Bn, T, Jn, Hn)
    keep = torch.ones(Dn, dtype=torch.bool, device=got.device)
    keep[bad * DH:(bad + 1) * DH] = False
    assert torch.isfinite(clean).all()
    assert torch.isfinite(got[:, keep]).all()
    assert torch.equal(got[:, keep], clean[:, keep])
    assert torch.isnan(got[:, ~keep]).all()


@pytest.mark.parametrize("DH", WIDTHS)
@pytest.mark.parametrize("form,_b,T,Jn,temporal", FORMS, ids=[f[0] for f in FORMS])
def test_a_nan_batch_element_does_not_reach_its_neighbour(form, _b, T, Jn, temporal, DH):
    E = _eng()
    Bn, Hn, Dn = 2, 8, 8 * DH
    qkv = hashed(f"isoqkv{T}_{Jn}_{Dn}_{Bn}", (Bn * T * Jn, 3 * Dn), 21, 2.0).cuda()
    bad = qkv.clone()
    bad[T * Jn:] = float("nan")
    alone = _run_form(E, form, qkv[:T * Jn].contiguous(), 1, T, Jn, Hn)
    both = _run_form(E, form, bad, Bn, T, Jn, Hn)
    assert torch.isfinite(both[:T * Jn]).all()
    assert torch.equal(both[:T * Jn], alone)


# ------------------------------------------------------------------------------------------------ 6. sharp softmax
@pytest.mark.parametrize("DH", WIDTHS)
@pytest.mark.parametrize("Bn,T,Jn,temporal,stream", [(2, 7, 17, False, False), (1, 100, 3, True, False), (1, 300, 3, True, True)],
                         ids=["spatial", "resident", "streaming"])
def test_sharp_softmax(Bn, T, Jn, temporal, stream, DH):
    """Logits up to ~100 (near one-hot rows): the bound of tests/test_gpu_ops.py::test_attention_fast_kernels_agree_with_generic_on_sharp_softmax."""
    E = _eng()
    Hn, Dn = 8, 8 * DH
    qkv = hashed(f"sharp{T}_{Dn}", (Bn * T * Jn, 3 * Dn), 22, 9.0).cuda()
    ref = attn_ref(qkv, Bn, T, Jn, Hn, temporal).cpu()
    a = E.op_attention_long_f32_hx(qkv, Bn, T, Jn, Hn) if stream else E.op_attention_f32_hx(qkv, Bn, T, Jn, Hn, temporal)
    b = E.op_attention(qkv, Bn, T, Jn, Hn, temporal, force_generic=True)
    print(f"attn_f32_hx sharp dh={DH} T={T} J={Jn}: new {maxabs(a, ref):.3e} generic {maxabs(b, ref):.3e} apart {maxabs(a, b.cpu()):.3e}")
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert maxabs(a, ref) < 2e-3 and maxabs(b, ref) < 2e-3
    assert maxabs(a, b.cpu()) < 2e-3


# ------------------------------------------------------------------------------------------------ 7. refusals
@pytest.mark.parametrize("T,Jn,Dn,Hn,temporal", [(27, 2, 256, 8, True), (27, 2, 512, 8, True), (27, 2, 1024, 8, True),
                                                 (257, 2, 384, 8, True), (193, 2, 768, 8, True),
                                                 (1, 257, 384, 8, False), (1, 193, 768, 8, False)],
                         ids=["width32", "width64", "width128", "257frames_dh48", "193frames_dh96", "257joints_dh48", "193joints_dh96"])
def test_resident_entry_refuses(T, Jn, Dn, Hn, temporal):
    qkv = torch.zeros((T * Jn, 3 * Dn), device="cuda")
    with pytest.raises(D3DError, match="head_dim 48 or 96"):
        _eng().op_attention_f32_hx(qkv, 1, T, Jn, Hn, temporal)


@pytest.mark.parametrize("Dn,Hn", [(256, 8), (512, 8), (1024, 8)], ids=["width32", "width64", "width128"])
def test_streaming_entry_refuses_other_widths(Dn, Hn):
    qkv = torch.zeros((27 * 2, 3 * Dn), device="cuda")
    with pytest.raises(D3DError, match="head_dim 48 or 96"):
        _eng().op_attention_long_f32_hx(qkv, 1, 27, 2, Hn)


# ------------------------------------------------------------------------------------------------ 8. - 12. engine level
EMBED = [384, 768]


def _cfg(T, Dn, Jn=17, Hn=8):
    return DenoiserConfig(num_frame=T, num_joints=Jn, embed_dim=Dn, depth=DEPTH, num_heads=Hn)


def _sd(cfg, seed=11):   # this module's weights: seed 11 of the trained-like family
    return torch_sd(cfg, seed, family="trainedlike")


def _net(cfg, seed=11, prec="fp32"):
    return build_net(cfg, seed, prec, family="trainedlike")


def _product(cfg, seed=11, prec="fp32", sampling=2):   # this module's defaults; the weights of _sd
    return product_with_engine(cfg, seed, prec, sampling, family="trainedlike")


def _sample(eng, x2d, nz):   # reads this feature's proof-of-path key, LAST
    out = eng.ddim_sample(x2d, nz).clone()
    return out, eng.info(LAST)


def _others(eng):
    return [eng.info(k) for k in OTHER_LAST]


@pytest.mark.parametrize("Dn,T,want", [(384, 27, 3), (768, 27, 3), (384, 300, 5), (768, 243, 5)])
def test_forward_denoise_against_the_oracle_with_the_option_on_and_off(Dn, T, want):
    """forward_denoise of an FP32 engine at B = 2, trained-like weights, depth 1, per-row t, against oracle/d3d_oracle.py in fp64: the
    kernels of these widths (T = 27: both block types resident; T = 300 at width 48 and T = 243 > 192 at width 96: the temporal blocks
    streaming) and the generic kernel both inside the project's 1e-4 gate."""
    from oracle import d3d_oracle as orc
    cfg = _cfg(T, Dn)
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
    assert eng.info(LAST) == 0                         # before any forward
    eng.range_flags(clear=True)
    err = {}
    try:
        for opt in (1, 0):
            eng.set_option(KEY, opt)
            out = net.forward_denoise(xcat.cuda(), t.cuda())
            assert eng.info(LAST) == (want if opt else 0)
            assert _others(eng) == [0] * len(OTHER_LAST)
            err[opt] = (out.cpu().double() - ref64).abs().max().item()
    finally:
        eng.set_option(KEY, default)
    print(f"attn_f32_hx D={Dn} T={T} B=2: err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}")
    assert eng.range_flags() == 0
    assert err[1] <= GATE and err[0] <= GATE


@pytest.mark.parametrize("Dn", EMBED)
def test_rows_do_not_depend_on_batch_streams_workspace_contents_or_graph_replay(Dn):
    T, Bn = 27, 3
    _, _, eng = _product(_cfg(T, Dn))
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


@pytest.mark.parametrize("Dn,T,Jn,want", [(768, 27, 193, 2), (384, 300, 17, 5)])
def test_each_block_type_decides_alone(Dn, T, Jn, want):
    """193 joints at width 96: the spatial blocks stay on k_attn_generic, the temporal ones run the resident kernel; 300 frames at width
    48: the spatial blocks resident, the temporal ones streaming."""
    _, _, eng = _product(_cfg(T, Dn, Jn=Jn))
    eng.set_option(KEY, 1)
    assert eng.info(LAST) == 0                     # before any forward
    out, last = _sample(eng, *xy(1, T, 83, Jn))
    assert last == want and torch.isfinite(out).all()
    assert _others(eng) == [0] * len(OTHER_LAST)


def test_engines_with_heads_of_64_columns_ignore_the_option():
    T = 27
    _, _, eng = _product(_cfg(T, 512))
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


@pytest.mark.parametrize("Dn", EMBED)
def test_f16x3_engines_are_left_alone(Dn):
    """Neither flow of an F16X3 engine at embed_dim 384 / 768 -- the folded one on the F16X3 kernels of these widths, the plain one
    "attn_hx" = 0 selects (which calls the same attention dispatch with the generic kernel) -- takes the fp32 kernels, and neither changes
    a bit."""
    T = 27
    _, _, e3 = _product(_cfg(T, Dn), prec="f16x3")
    x2d, nz = xy(1, T, 83)
    default, flow_default = e3.info(KEY), e3.info("attn_hx")
    assert e3.info(LAST) == 0
    try:
        for flow in (1, 0):
            e3.set_option("attn_hx", flow)
            res = {}
            for opt in (1, 0):
                e3.set_option(KEY, opt)
                res[opt] = e3.ddim_sample(x2d, nz).clone()
                assert e3.info("attn_hx_last") == (3 if flow else 0) and e3.info(LAST) == 0
            assert torch.isfinite(res[1]).all() and torch.equal(res[1], res[0])
    finally:
        e3.set_option("attn_hx", flow_default)
        e3.set_option(KEY, default)


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_one_head_of_48_columns_keeps_the_generic_kernel(prec):
    """embed_dim 48 is no multiple of 32: the plan leaves such an engine on the generic kernel in both precisions (they must agree bit for
    bit: tests/test_gpu_attn_hx_engine.py), whatever the option says."""
    T = 27
    _, _, eng = _product(_cfg(T, 48, Hn=1), prec=prec)
    x2d, nz = xy(1, T, 85)
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


def test_the_auto_fallback_engine_runs_the_kernels():
    """precision "auto" at T = 27, embed_dim 384: an input scaled past the plane range raises the F16X3 guard, the call is repeated on the
    exact-fp32 engine -- ONE warning, the fp32 model's result bit for bit, and that engine's blocks on the kernels for heads of 48
    columns."""
    T, Bn = 27, 2
    cfg = _cfg(T, 384)
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
