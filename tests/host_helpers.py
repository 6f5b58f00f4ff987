"""Shared helpers of the host-side tests: engines that exist on the host only (created through the C ABI, never committed) and their
info keys.  No GPU needed."""
import ctypes as C

import pytest

from diff3dhpe_amd import _lib
from diff3dhpe_amd.spec import DenoiserConfig


def create_host_engine(prec, **cfg_kwargs):
    """The handle of an engine of DenoiserConfig(**cfg_kwargs) in precision `prec`; the caller destroys it."""
    cfg = DenoiserConfig(**cfg_kwargs)
    c = _lib.Config(cfg.num_frame, cfg.num_joints, cfg.in_chans, cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.mlp_hidden,
                    int(cfg.with_time_emb), int(cfg.seq2frame), _lib.PRECISIONS[prec])
    h = C.c_void_p()
    assert _lib.lib().d3d_engine_create(C.byref(c), C.byref(h)) == 0
    return h


def host_engine_fixture(prec="f16x3", **cfg_kwargs):
    """A pytest fixture that yields (L, h) of such an engine and destroys it at teardown; each module binds its own:
    host_engine = host_engine_fixture(num_frame=243, embed_dim=256, prec="fp32")."""
    @pytest.fixture()
    def host_engine():
        L = _lib.lib()
        h = create_host_engine(prec, **cfg_kwargs)
        yield L, h
        L.d3d_engine_destroy(h)
    return host_engine


def engine_info(L, h, key, sentinel=-1):
    """(rc, value) of d3d_engine_get_info; `sentinel` is what value holds when the call writes nothing."""
    v = C.c_int64(sentinel)
    rc = L.d3d_engine_get_info(h, key.encode(), C.byref(v))
    return rc, int(v.value)
