"""mi_cvec_load (loadControlVector, ControlVector.cpp:20-98) on files written by
synthetic.write_cvec_gguf: data[n_embd*(N-1) + j] += src[j] * strength over the direction.N
tensors, and every malformed file refused.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from blama_amd import engine, synthetic

D = 64


def _v(seed, n=D):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def test_two_files_summed_with_their_strengths(tmp_path):
    a, b = str(tmp_path / "a.gguf"), str(tmp_path / "b.gguf")
    synthetic.write_cvec_gguf(a, {1: _v(1), 2: _v(2)})
    synthetic.write_cvec_gguf(b, {2: _v(3), 3: _v(4)})
    da, na = engine.cvec_load(a, 0.5)
    db, nb = engine.cvec_load(b, -2.0)
    assert na == nb == D and da.size == 2 * D and db.size == 3 * D
    s05, sm2 = np.float32(0.5), np.float32(-2.0)
    assert np.array_equal(da, np.concatenate([_v(1) * s05, _v(2) * s05]))
    assert np.array_equal(db, np.concatenate([np.zeros(D, np.float32), _v(3) * sm2, _v(4) * sm2]))
    # the ABI accumulates into the caller's buffer: both files into one
    both = np.zeros(3 * D, np.float32)
    ne = C.c_int32()
    for path, s in ((a, 0.5), (b, -2.0)):
        assert engine.lib().mi_cvec_load(path.encode(), s, both.ctypes.data_as(C.POINTER(C.c_float)), both.size,
                                         C.byref(ne)) > 0
    want = np.zeros(3 * D, np.float32)
    want[:2 * D] += da
    want += db
    assert np.array_equal(both, want)


def test_same_layer_twice_accumulates(tmp_path):
    p = str(tmp_path / "c.gguf")
    synthetic.write_cvec_gguf(p, [(2, _v(5)), (1, _v(6)), (2, _v(7))])
    d, n = engine.cvec_load(p, 1.5)
    s = np.float32(1.5)
    assert n == D and np.array_equal(d[:D], _v(6) * s)
    assert np.array_equal(d[D:], _v(5) * s + _v(7) * s)


def test_gap_in_layers_is_zeros_and_size_query(tmp_path):
    p = str(tmp_path / "g.gguf")
    synthetic.write_cvec_gguf(p, {1: _v(8), 4: _v(9)})
    d, n = engine.cvec_load(p, 1.0)
    assert d.size == 4 * D and not d[D:3 * D].any()
    assert np.array_equal(d[:D], _v(8)) and np.array_equal(d[3 * D:], _v(9))
    # data NULL is a size query; a buffer that is too small is left untouched
    ne = C.c_int32()
    L = engine.lib()
    assert L.mi_cvec_load(p.encode(), 1.0, None, 0, C.byref(ne)) == 4 * D and ne.value == D
    small = np.full(2 * D, 7.0, np.float32)
    assert L.mi_cvec_load(p.encode(), 1.0, small.ctypes.data_as(C.POINTER(C.c_float)), small.size, None) == 4 * D
    assert np.all(small == 7.0)


@pytest.mark.parametrize("what,tensors", [
    ("layer 0", [(0, _v(1))]),
    ("negative layer", [("direction.-3", _v(1))]),
    ("unparsable layer", [("direction.x", _v(1))]),
    ("no layer", [("direction", _v(1))]),
    ("another name", [(1, _v(1)), ("token_embd.weight", _v(2))]),
    ("non-F32", [(1, _v(1).astype(np.float16))]),
    ("not 1-D", [(1, _v(1, 2 * D).reshape(2, D))]),
    ("differing lengths", [(1, _v(1)), (2, _v(2, D // 2))]),
])
def test_invalid_files_are_refused(tmp_path, what, tensors):
    p = str(tmp_path / "bad.gguf")
    synthetic.write_cvec_gguf(p, tensors)
    assert engine.lib().mi_cvec_load(p.encode(), 1.0, None, 0, None) < 0, what
    assert engine.last_error()
    with pytest.raises(engine.EngineError, match="cvec_load"):
        engine.cvec_load(p)


def test_unreadable_file_is_refused(tmp_path):
    assert engine.lib().mi_cvec_load(str(tmp_path / "missing.gguf").encode(), 1.0, None, 0, None) < 0
    assert "cannot open" in engine.last_error()
    p = tmp_path / "junk.gguf"
    p.write_bytes(b"NOPE" + bytes(64))
    assert engine.lib().mi_cvec_load(str(p).encode(), 1.0, None, 0, None) < 0
