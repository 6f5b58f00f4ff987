"""The attention plan -- the flow, the kernel family of the spatial and of the temporal blocks, whether the temporal blocks stream -- and
the twelve "*_last" info keys derived from it, over a grid of engines, windows, joint counts and option sets, against the choices of the
library as it stood before the plan became a table (csrc/attn_dispatch.h).  attn_choose() and attn_plan_key() are plain host functions
of the library, reached through their C++ symbols as the predicate tests reach theirs.  No GPU needed.

tests/golden/attention_plan_grid.npz was recorded once from that earlier library, not from this code: a throwaway export appended to a
scratch copy of its engine.hip built a d3d_engine on the host, set precision, T, J, D, H, the twelve attention options and
"fold_layernorm", gave it two default blocks, called its plan_blocks(&e, 1) and its attention_plan_info for every key.  The file holds
the axes (engines = (precision, embed_dim, heads); T; J; optsets = (attention option bits in the order of `options`, fold_layernorm)),
the names (flows, kernels: family, "_long" = key-streaming; key_names), plan[engine, T, J, optset] = (flow, spatial kernel, temporal
kernel) and keys[engine, T, J, optset, key]."""
import ctypes as C
import os

import numpy as np

from diff3dhpe_amd import _lib

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_plan_grid.npz"))


class Pick(C.Structure):
    _fields_ = [("family", C.c_int), ("stream", C.c_int)]


class Choice(C.Structure):
    _fields_ = [("flow", C.c_int), ("sp", Pick), ("tp", Pick)]


def _cxx(symbol, restype, argtypes):
    f = getattr(_lib.lib(), symbol)
    f.restype, f.argtypes = restype, argtypes
    return f


def _api():
    choose = _cxx("_ZN3d3d11attn_chooseEijbiiii", Choice, [C.c_int, C.c_uint, C.c_bool] + [C.c_int] * 4)
    key = _cxx("_ZN3d3d13attn_plan_keyERKNS_10AttnChoiceEPKcPl", C.c_bool, [C.POINTER(Choice), C.c_char_p, C.POINTER(C.c_int64)])
    name = _cxx("_ZN3d3d16attn_family_nameEi", C.c_char_p, [C.c_int])
    option = _cxx("_ZN3d3d17attn_option_indexEPKc", C.c_int, [C.c_char_p])
    defaults = _cxx("_ZN3d3d20attn_option_defaultsEv", C.c_uint, [])
    return choose, key, name, option, defaults


def test_the_grid_is_the_one_the_issue_asks_for():
    eng = {tuple(e) for e in G["engines"].tolist()}
    widths = [(16, h) for h in (1, 2, 4, 8)] + [(32, h) for h in (1, 2, 3, 8)] + [(48, h) for h in (1, 2, 3, 8)] + \
             [(w, h) for w in (64, 96, 128) for h in (1, 8)]
    assert eng == {(p, w * h, h) for p in (0, 1) for w, h in widths} | {(0, 64, 8), (1, 64, 8), (2, 512, 8)}
    assert set(G["T"].tolist()) >= {1, 27, 127, 128, 129, 192, 193, 243, 255, 256, 257, 300}
    assert G["J"].tolist() == [1, 15, 16, 17, 18, 33, 128, 129, 192, 193, 256, 257]
    every = (1 << 12) - 1
    assert {tuple(o) for o in G["optsets"].tolist()} == {(every, 1), (every, 0), (0, 1)} | {(every ^ (1 << i), 1) for i in range(12)}
    assert len(G["options"]) == 12 and len(G["key_names"]) == 12
    assert G["plan"].shape == (len(G["engines"]), len(G["T"]), len(G["J"]), len(G["optsets"]), 3)
    assert G["keys"].shape == G["plan"].shape[:4] + (12,)


def test_option_bits_and_defaults():
    _, _, _, option, defaults = _api()
    assert [option(k.encode()) for k in G["options"].tolist()] == list(range(12))       # the golden's bit order is the table's
    assert option(b"fold_layernorm") == -1 and option(b"attn_h32_last") == -1
    assert defaults() == (1 << 12) - 1                                                  # every attention option is on by default


def test_every_grid_point_matches_the_recorded_plan():
    choose, key, name, _, _ = _api()
    flows, kernels = G["flows"].tolist(), G["kernels"].tolist()
    assert flows == ["plain", "fold", "bf16"]
    families = []
    while name(len(families)) is not None:
        families.append(name(len(families)).decode())
    assert {f + s for f in families for s in ("", "_long")} >= set(kernels)
    key_names = [k.encode() for k in G["key_names"].tolist()]
    plan, keys = G["plan"], G["keys"]
    value = C.c_int64()
    bad, points = [], 0
    for a, (prec, D, H) in enumerate(G["engines"].tolist()):
        for b, T in enumerate(G["T"].tolist()):
            for c, J in enumerate(G["J"].tolist()):
                for o, (bits, fold) in enumerate(G["optsets"].tolist()):
                    ch = choose(prec, bits, bool(fold), T, J, D, H)
                    assert not ch.sp.stream                                             # only temporal blocks stream
                    got = (ch.flow, kernels.index(families[ch.sp.family]),
                           kernels.index(families[ch.tp.family] + ("_long" if ch.tp.stream else "")))
                    got_keys = []
                    for k in key_names:
                        assert key(C.byref(ch), k, C.byref(value))
                        got_keys.append(value.value)
                    points += 1
                    if got != tuple(plan[a, b, c, o].tolist()) or got_keys != keys[a, b, c, o].tolist():
                        bad.append(((prec, D, H, T, J, bits, fold), got, plan[a, b, c, o].tolist(), got_keys, keys[a, b, c, o].tolist()))
    assert points == plan[..., 0].size
    assert not bad, (len(bad), bad[:5])


def test_keys_are_zero_before_any_forward_and_unknown_keys_are_refused():
    _, key, _, _, _ = _api()
    value = C.c_int64(7)
    fresh = Choice()                                                                    # the zeroed plan of a new engine
    for k in G["key_names"].tolist():
        assert key(C.byref(fresh), k.encode(), C.byref(value)) and value.value == 0, k
    assert not key(C.byref(fresh), b"fused_spatial_last", C.byref(value))
    assert not key(C.byref(fresh), b"attn_h32", C.byref(value))
