"""The group-length axis of the attention kernels, as plain integer arithmetic: which lengths the sweeps of
tests/test_gpu_group_lengths.py run and which kernel form each length selects.  No GPU, no torch: tests/test_group_lengths_host.py
checks these tables against a literal restatement of the library's predicates, so a sweep cannot shrink unnoticed.

N is the group length: the frame count T in temporal blocks, the joint count J in spatial ones."""

KEY_TILE = 32            # keys per key tile of every MFMA attention kernel
RESIDENT_MAX = 256       # the longest group whose keys stay in LDS (8 key tiles); longer ones stream 256-key chunks
FUSED_ROWS = 255         # rows of a 256-row tile of the fused temporal kernel that hold tokens
SMALL_ROWS = 127         # the same of a 128-row tile of the small-tile kernel


def nkt(N):
    """Key tiles of a group of N keys."""
    return (N + KEY_TILE - 1) // KEY_TILE


def pad_keys(N):
    """Pad keys in the last key tile."""
    return nkt(N) * KEY_TILE - N


def chunks(N):
    """256-key chunks the key-streaming kernels walk."""
    return (N + RESIDENT_MAX - 1) // RESIDENT_MAX


def grouped_G(T, J):
    """Joints per 256-row tile of the grouped fused temporal form (2 <= T <= 127)."""
    return min(FUSED_ROWS // T, J)


def grouped_TPS(T, J):
    """Tiles per batch element of the grouped form."""
    G = grouped_G(T, J)
    return (J + G - 1) // G


def small_groups_per_tile(N):
    """Whole groups per 128-row tile of the small-tile kernel."""
    return SMALL_ROWS // N


def temporal_path(T):
    """The temporal blocks of the default F16X3 flow at embed_dim 512 / 8 heads: "grouped" and "single" are the two forms of the fused
    qkv + attention kernel, "two_kernel" the qkv GEMM followed by the resident attention kernel, "long" by the key-streaming one."""
    if T > RESIDENT_MAX:
        return "long"
    if 2 <= T <= 127:
        return "grouped"
    if 193 <= T <= 255:
        return "single"
    return "two_kernel"


def fused_temporal(T):
    return temporal_path(T) in ("grouped", "single")


def fused_spatial(J):
    return J in (15, 16, 17)


# ------------------------------------------------------------------------------------------------ engine level: window lengths at 17 joints
ENGINE_GROUPED = [2, 8, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 36, 37, 42, 43, 51, 52, 63, 64, 85, 86, 127]
ENGINE_TILE_EDGES = [33, 65, 95, 96, 97]
ENGINE_TWO_KERNEL = [128, 129, 159, 160, 161, 191, 192]
ENGINE_SINGLE = [193, 194, 223, 224, 225, 254, 255]
ENGINE_T = sorted(ENGINE_GROUPED + ENGINE_TILE_EDGES + ENGINE_TWO_KERNEL + ENGINE_SINGLE + [256, 257])
# (T, J): 255-row tiles at 15 / 16 joints (the spatial fused kernel on 16-frame tiles, G = min(255 / T, J)); 21 joints: two-kernel spatial
# blocks, five temporal tiles per batch element
ENGINE_OTHER_JOINTS = [(51, 15), (51, 16), (85, 15), (85, 16), (43, 21)]
ENGINE_CASES = [(T, 17) for T in ENGINE_T] + ENGINE_OTHER_JOINTS


# ------------------------------------------------------------------------------------------------ op level: the lengths of every hook
def _around_multiples(last):
    return sorted({n for m in range(KEY_TILE, last + 1, KEY_TILE) for n in (m - 1, m, m + 1)})


_LONG = list(range(1, 65)) + list(range(255, 291)) + [511, 512, 513, 545, 768, 769]
SWEEPS = {
    "fp32": list(range(1, 257)),
    "fp32_generic": _around_multiples(256),          # 31, 32, 33, ... 255, 256, 257
    "f16x3": list(range(1, 257)),
    "f16x3_spatial": list(range(1, 33)),
    "h32": list(range(1, 257)),
    "h32_spatial": list(range(1, 33)),
    "long": _LONG,
    "long_f32": _LONG,
    "bf16": list(range(1, 257)),
    "small": list(range(1, 128)),
    "qkv_bf16": list(range(1, 256)),
    "qkv_bf16_spatial": list(range(1, 33)),
}
SMALL_SPATIAL = [(N, groups) for N in (15, 16, 17) for groups in (1, 7, 8, 9, 20)]


def classes(hook):
    """[(class id, lengths)]: a sweep split by key-tile count -- by 256-key chunk beyond the resident range, where the class id is
    100 x chunks so that it cannot be taken for a key-tile count."""
    out = {}
    for N in SWEEPS[hook]:
        out.setdefault(nkt(N) if N <= RESIDENT_MAX else 100 * chunks(N), []).append(N)
    return sorted(out.items())


def class_params(hook):
    """(hook, class id) pairs for pytest.mark.parametrize."""
    return [(hook, c) for c, _ in classes(hook)]


def class_lengths(hook, c):
    return dict(classes(hook))[c]
