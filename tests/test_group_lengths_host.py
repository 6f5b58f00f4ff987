"""tests/group_lengths.py against the library's rules (no GPU): the sweeps of tests/test_gpu_group_lengths.py reach every regime of the
group-length axis, and the path that file expects per window length is the one the predicates of plan_blocks select -- restated here
literally, and asked of the library's own host functions (reached through their C++ symbols)."""
import ctypes as C

import group_lengths as gl
from diff3dhpe_amd import _lib

D, H = 512, 8


# literal restatements: kernels_qkv_tattn.hip, kernels_attn_x3.hip, kernels_attn_x3_long.hip, plan_blocks (engine.hip)
def qkv_tattn_ok(T, J, D, H, K):
    return ((T > 192 and T <= 255) or (T >= 2 and T <= 127)) and J >= 1 and H == 8 and D == 512 and K % 64 == 0 and K >= 128


def attn_temporal_x3_ok(T, D, H):
    return T >= 1 and T <= 256 and H > 0 and D == H * 64


def attn_temporal_x3_long_ok(T, D, H):
    return T >= 1 and H > 0 and D == H * 64


def tp_long(T, D, H):
    return T > 256 and attn_temporal_x3_long_ok(T, D, H)


def _path(tattn_ok, x3_ok, long_ok, T, J):
    if T > 256 and long_ok(T, D, H):
        return "long"
    assert x3_ok(T, D, H), T                     # (else the engine leaves the folded flow altogether)
    if tattn_ok(T, J, D, H, D):
        return "grouped" if T <= 127 else "single"
    return "two_kernel"


def _cxx(name, nargs):
    f = getattr(_lib.lib(), f"_ZN3d3d{len(name)}{name}E" + "i" * nargs)
    f.restype, f.argtypes = C.c_bool, [C.c_int] * nargs
    return f


def test_expected_path_agrees_with_the_restated_predicates():
    assert tp_long(257, D, H) and not tp_long(256, D, H)
    for T in range(1, 400):
        for J in (15, 16, 17, 21):
            assert gl.temporal_path(T) == _path(qkv_tattn_ok, attn_temporal_x3_ok, attn_temporal_x3_long_ok, T, J), (T, J)
            assert gl.fused_temporal(T) == qkv_tattn_ok(T, J, D, H, D)


def test_expected_path_agrees_with_the_library():
    tattn, x3, lng = _cxx("qkv_tattn_ok", 5), _cxx("attn_temporal_x3_ok", 3), _cxx("attn_temporal_x3_long_ok", 3)
    sattn = _cxx("qkv_sattn_ok", 4)
    for T in range(1, 400):
        assert gl.temporal_path(T) == _path(tattn, x3, lng, T, 17), T
    for J in range(1, 40):
        assert gl.fused_spatial(J) == bool(sattn(J, D, H, D)), J


def test_engine_list_holds_both_ends_of_every_joints_per_tile_class():
    by_G = {}
    for T in range(2, 128):
        by_G.setdefault(gl.grouped_G(T, 17), []).append(T)
    assert sorted(by_G) == [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 17]        # (no T gives 16: 255 // 15 = 17, 255 // 16 = 15)
    for G, Ts in by_G.items():
        assert min(Ts) in gl.ENGINE_T and max(Ts) in gl.ENGINE_T, (G, min(Ts), max(Ts))
    # a joint's keys ending on a key-tile boundary, and tiles filled to the last row
    assert {32, 64, 96} <= set(gl.ENGINE_T)
    assert [T for T in gl.ENGINE_T if T <= 127 and gl.grouped_G(T, 17) * T == gl.FUSED_ROWS] == [15, 17, 51, 85]
    # tiles per batch element: every count the grouped form reaches at 17 joints appears
    assert {gl.grouped_TPS(T, 17) for T in range(2, 128)} == {gl.grouped_TPS(T, 17) for T in gl.ENGINE_T if T <= 127}
    assert (gl.grouped_G(43, 21), gl.grouped_TPS(43, 21)) == (5, 5)
    assert [(gl.grouped_G(T, J), gl.grouped_TPS(T, J)) for T, J in gl.ENGINE_OTHER_JOINTS[:4]] == [(5, 3), (5, 4), (3, 5), (3, 6)]


def test_engine_list_holds_every_multiple_of_32_with_both_neighbours():
    for m in range(32, 257, 32):
        assert {m - 1, m, m + 1} <= set(gl.ENGINE_T), m


def test_engine_list_reaches_every_path_and_both_sides_of_every_switch():
    assert {gl.temporal_path(T) for T in gl.ENGINE_T} == {"grouped", "single", "two_kernel", "long"}
    for lo in (127, 192, 255, 256):              # the lengths behind which the plan switches kernels
        assert gl.temporal_path(lo) != gl.temporal_path(lo + 1) and {lo, lo + 1} <= set(gl.ENGINE_T)
    assert len(set(gl.ENGINE_CASES)) == len(gl.ENGINE_CASES)
    assert {J for _, J in gl.ENGINE_CASES} == {15, 16, 17, 21}


def test_op_sweeps_cover_every_key_tile_count_and_pad_count():
    every = {(k, p) for k in range(1, 9) for p in range(32)}
    for hook in ("fp32", "f16x3", "h32", "bf16"):
        assert {(gl.nkt(N), gl.pad_keys(N)) for N in gl.SWEEPS[hook]} == every, hook
    assert {(gl.nkt(N), gl.pad_keys(N)) for N in gl.SWEEPS["qkv_bf16"]} == every - {(8, 0)}        # 255 rows per tile
    assert {(gl.nkt(N), gl.pad_keys(N)) for N in gl.SWEEPS["small"]} == {(k, p) for k, p in every if k <= 4} - {(4, 0)}
    for hook in ("f16x3_spatial", "h32_spatial", "qkv_bf16_spatial"):
        assert {(gl.nkt(N), gl.pad_keys(N)) for N in gl.SWEEPS[hook]} == {(1, p) for p in range(32)}, hook
    assert set(gl.SWEEPS["fp32_generic"]) == {n for m in range(32, 257, 32) for n in (m - 1, m, m + 1)}
    # the key-streaming kernels: the range shared with the resident kernels, then one, two and three whole chunks with a remainder of
    # none, one key, one key tile + 1 and a whole chunk - 1
    for hook in ("long", "long_f32"):
        s = set(gl.SWEEPS[hook])
        assert set(range(1, 65)) | set(range(255, 291)) | {511, 512, 513, 545, 768, 769} == s
        assert {gl.chunks(N) for N in s} == {1, 2, 3, 4}
    assert {gl.small_groups_per_tile(N) for N in gl.SWEEPS["small"]} == {127 // N for N in range(1, 128)}
    assert gl.SMALL_SPATIAL == [(N, g) for N in (15, 16, 17) for g in (1, 7, 8, 9, 20)]


def test_classes_partition_every_sweep():
    for hook, lengths in gl.SWEEPS.items():
        cl = gl.classes(hook)
        assert sorted(N for _, Ns in cl for N in Ns) == sorted(lengths), hook
        assert all(len(Ns) <= 36 for _, Ns in cl), hook              # a test loops over one class: it stays short
        for c, Ns in cl:
            assert all((gl.nkt(N) if N <= 256 else 100 * gl.chunks(N)) == c for N in Ns)
    assert [c for c, _ in gl.classes("f16x3")] == list(range(1, 9))
    assert [c for c, _ in gl.classes("long")] == [1, 2, 8, 200, 300, 400]
    assert gl.class_params("small") == [("small", c) for c in (1, 2, 3, 4)]
    assert gl.class_lengths("fp32_generic", 200) == [257]
