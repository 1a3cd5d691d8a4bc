"""CPU: the presentation builders of tests/presentation_cases.py produce what
they claim, and the mirrors state an element type at every pointer hand-over.

1 every builder really yields the form its id names (strides, flags, dtypes,
  shared memory) and round-trips to the baseline values exactly;
2 mmb_lib.ptr / mmb_lib.rows_ptr / latent._ptr_array reject a host tensor, a
  non-contiguous tensor and a wrong element type with MMBError (pure host
  checks: no library call);
3 by `ast`: every `L.ptr(` in the package passes a dtype, every
  `L.call("mmb_*", ...)` whose arguments resolve positionally states, per
  pointer parameter, the pointee type include/mmb.h declares, and no bare
  `.data_ptr()` is handed to the library outside mmb_lib.
"""
import ast
import os

import numpy as np
import pytest
import torch

import latent as LT
import mmb_lib as L
import presentation_cases as PC
from abi_cases import ROOT, prototypes

PKG = os.path.join(ROOT, "multimodal-baselines_amd")


# ---------------------------------------------------------------- 1 the builders
def _base2(dtype=np.float32):
    return np.arange(1, 7 * 5 + 1, dtype=dtype).reshape(7, 5)


def test_numpy_builders_produce_their_forms():
    a = _base2()
    assert a.flags.c_contiguous
    b = PC.n_float64(a)
    assert b.dtype == np.float64 and b.flags.c_contiguous
    b = PC.n_fortran(a)
    assert b.flags.f_contiguous and not b.flags.c_contiguous and b.strides == (4, 28)
    b = PC.n_stepped(a)
    assert b.strides == (2 * 11 * 4, 8) and not b.flags.c_contiguous and b.base is not None
    assert np.isnan(b.base).sum() == b.base.size - a.size  # the filler around the view
    b = PC.n_negative(a)
    assert b.strides == (-20, 4) and not b.flags.c_contiguous
    b = PC.n_readonly(a)
    assert not b.flags.writeable and b.flags.c_contiguous and not np.shares_memory(a, b)
    v = np.arange(9, dtype=np.float64)
    assert PC.n_stepped(v).strides == (16,) and PC.n_negative(v).strides == (-8,)
    for k, f in PC.NUMPY_FORMS.items():
        for base in (a, v):
            got = f(base)
            assert not np.shares_memory(got, base), k
            assert got.shape == base.shape and np.array_equal(got.astype(base.dtype), base), k


def test_numpy_id_and_mask_forms():
    ids = np.arange(35, dtype=np.int64).reshape(7, 5)
    forms = dict(PC.numpy_forms(ids, ids=True))
    assert set(forms) == {"N2", "N3", "N4", "N6", "N5-int32", "N5-int16", "N5-uint8", "N5-list"}
    assert forms["N5-int32"](ids).dtype == np.int32 and forms["N5-int16"](ids).dtype == np.int16
    assert forms["N5-uint8"](ids).dtype == np.uint8
    as_list = forms["N5-list"](ids)
    assert isinstance(as_list, list) and isinstance(as_list[0], list) and isinstance(as_list[0][0], int)
    for k, f in forms.items():
        assert np.array_equal(np.asarray(f(ids)), ids), k
    assert "N5-uint8" not in dict(PC.numpy_forms(ids + 300, ids=True))
    assert [k for k, _ in PC.numpy_forms(np.zeros(4, np.float32))] == ["N1", "N3", "N4", "N6"]
    m = (np.arange(35).reshape(7, 5) % 3 > 0).astype(np.float32)
    kinds = {k: f(m).dtype.kind for k, f in PC.MASK_FORMS.items()}
    assert kinds == {"N7-bool": "b", "N7-int": "i", "N7-float": "f"}
    for f in PC.MASK_FORMS.values():
        assert np.array_equal(f(m) > 0, m > 0)


def test_torch_builders_produce_their_forms():
    t = torch.arange(1, 4 * 7 * 5 + 1, dtype=torch.float32).reshape(4, 7, 5)
    b = PC.t_float64(t)
    assert b.dtype == torch.float64 and b.is_contiguous()
    b = PC.t_colblock(t)
    assert b.stride() == (70, 10, 1) and not b.is_contiguous() and b.storage_offset() == 2
    b = PC.t_stepped(t)
    assert b.stride() == (70, 5, 1) and not b.is_contiguous()
    b = PC.t_transposed(t)
    assert b.stride() == (35, 1, 7) and not b.is_contiguous()
    assert PC.t_cpu(t).device.type == "cpu"
    ids = torch.arange(35).reshape(7, 5)
    assert PC.t_int32(ids).dtype == torch.int32 and PC.t_int64(ids).dtype == torch.int64
    assert PC.t_colblock(ids).stride() == (10, 1) and int(PC.t_colblock(ids)._base.sum()) == \
        int(ids.sum()) + 5 * 7  # integer filler: a valid id
    for k, f in PC.TORCH_FORMS.items():
        for base in (t, ids) if k != "T2" else (t,):
            got = f(base)
            assert got.shape == base.shape and torch.equal(got.to(base.dtype), base), k
            if k.startswith("T3"):
                assert got.data_ptr() != base.data_ptr() and not got.is_contiguous(), k
    # the filler of a float view is NaN, outside the view only
    assert not torch.isnan(PC.t_stepped(t)).any() and torch.isnan(PC.t_stepped(t)._base).sum() == t.numel()
    assert PC.torch_forms(t) == ["T2", "T3a", "T3b", "T3c"]
    assert PC.torch_forms(t[:, :1], cpu=True) == ["T1", "T2", "T3a", "T3b"]
    assert PC.torch_forms(ids, ids=True) == ["T3a", "T3b", "T3c", "T6-int32", "T6-int64"]
    ex = t[:1].expand(4, 7, 5)
    assert ex.stride(0) == 0 and torch.equal(ex[3], t[0])


def test_result_comparison_is_by_bits():
    a = torch.tensor([0.0, float("nan"), 1.0])
    assert PC.same_result(a.clone(), a)
    assert not PC.same_result(torch.tensor([-0.0, float("nan"), 1.0]), a)
    assert not PC.same_result(a.double(), a) and not PC.same_result(a[:2], a)
    n = np.array([1.0, 2.0])
    assert PC.same_result(n.copy(), n) and not PC.same_result(n.astype(np.float32), n)
    snap = PC.snapshot(a)
    assert PC.unchanged(a, snap)
    a[0] = 5.0
    assert not PC.unchanged(a, snap)


def test_case_inputs_are_f32_representable():
    z = PC.sif_inputs()
    for a in (z.We, z.w, z.weights, z.mask):
        assert np.array_equal(a.astype(np.float32).astype(a.dtype), a)
    assert z.ids.dtype == np.int64 and z.ids.max() < PC.SIF_V <= 255
    for n, d in PC.PC_SHAPES:
        X = PC.pc_rows(n, d)
        assert X.dtype == np.float32 and X.shape == (n, d)
        X64 = PC.pc_rows(n, d, False)
        assert not np.array_equal(X64.astype(np.float32).astype(np.float64), X64)
    assert PC.PC_SHAPES[0][0] >= PC.PC_SHAPES[0][1] and PC.PC_SHAPES[1][0] < PC.PC_SHAPES[1][1]


# ---------------------------------------------------------------- 2 the rejections
class _FakeDevice(torch.Tensor):
    """A host tensor that says it is on the device: lets the checks after the
    device check run on a machine without one.  Nothing reads its address."""

    @property
    def is_cuda(self):
        return True


def _fake(t):
    return t.as_subclass(_FakeDevice)


def test_ptr_rejects_host_strided_and_mistyped_tensors():
    host = torch.zeros(4, 6)
    with pytest.raises(L.MMBError, match="device"):
        L.ptr(host, L.F32)
    with pytest.raises(L.MMBError, match="contiguous"):
        L.ptr(_fake(host)[:, ::2], L.F32)
    with pytest.raises(L.MMBError, match="contiguous"):
        L.ptr(_fake(host).t(), L.F32)
    with pytest.raises(L.MMBError, match=r"torch\.float32.*torch\.float64"):
        L.ptr(_fake(host.double()), L.F32)
    with pytest.raises(L.MMBError, match=r"torch\.int32.*torch\.int64"):
        L.ptr(_fake(torch.zeros(3, dtype=torch.int64)), L.I32)
    with pytest.raises(L.MMBError, match=r"torch\.float16 or torch\.float32.*torch\.float64"):
        L.ptr(_fake(host.double()), L.S_BUF)
    # the wrong type is named before the device is looked at: a mistyped host tensor too
    with pytest.raises(L.MMBError, match="torch.float64"):
        L.ptr(host.double(), L.F32)
    assert L.ptr(None, L.F32) is None
    ok = _fake(host)
    assert L.ptr(ok, L.F32) == host.data_ptr() and L.ptr(ok, L.TABLE) == host.data_ptr()
    assert L.ptr(_fake(host.half()), L.FRAMES) is not None


def test_rows_ptr_keeps_the_unit_column_stride_rule():
    wide = torch.zeros(5, 12)
    blk = _fake(wide)[:, 2:8]
    assert L.rows_ptr(blk, L.F32, 6) == (wide.data_ptr() + 8, 12)
    assert L.rows_ptr(_fake(torch.zeros(5, 6)), L.F32, 6)[1] == 6
    assert L.rows_ptr(_fake(torch.zeros(1, 6)), L.F32, 6)[1] == 6
    with pytest.raises(L.MMBError, match="device"):
        L.rows_ptr(wide[:, 2:8], L.F32, 6)
    with pytest.raises(L.MMBError, match="torch.float64"):
        L.rows_ptr(_fake(wide.double())[:, 2:8], L.F32, 6)
    with pytest.raises(L.MMBError, match="stride"):  # a broadcast row: ld = 0 < F
        L.rows_ptr(_fake(torch.zeros(1, 6)).expand(5, 6), L.F32, 6)
    with pytest.raises(L.MMBError, match="stride"):  # column stride 2
        L.rows_ptr(_fake(wide)[:, ::2], L.F32, 6)
    with pytest.raises(L.MMBError, match="stride"):  # another width than the key's
        L.rows_ptr(_fake(wide)[:, 2:9], L.F32, 6)


def test_ptr_arrays_are_built_through_the_checks():
    good = _fake(torch.zeros(3, 3, 4, dtype=torch.float64))
    arr = LT._ptr_array([good, None, None], L.F64)
    assert arr[0] == good.data_ptr() and arr[1] is None and arr[2] is None
    with pytest.raises(L.MMBError, match="device"):
        LT._ptr_array([torch.zeros(3, 3, 4, dtype=torch.float64)], L.F64)
    with pytest.raises(L.MMBError, match="torch.float32"):
        LT._ptr_array([_fake(torch.zeros(3, 3, 4))], L.F64)
    with pytest.raises(L.MMBError, match="contiguous"):
        LT._ptr_array([good[:, :, ::2]], L.F64)
    mu = _fake(torch.zeros(5, 12))
    ptrs, lds = LT._rows_array([mu[:, :4], mu[:, 4:12]], L.F32, [4, 8])
    assert list(lds) == [12, 12] and ptrs[1] == mu.data_ptr() + 16
    with pytest.raises(L.MMBError, match="device"):
        LT._rows_array([torch.zeros(5, 4)], L.F32, [4])
    with pytest.raises(L.MMBError, match="torch.float64"):
        LT._rows_array([_fake(torch.zeros(5, 4, dtype=torch.float64))], L.F32, [4])
    with pytest.raises(L.MMBError, match="differ"):  # a gradient block at another row stride
        LT._rows_array([_fake(torch.zeros(5, 4))], L.F32, [4], lds=(12,))
    ptrs, lds = LT._rows_array([None, mu[:, :4]], L.F32, [8, 4], lds=(12, 12))
    assert ptrs[0] is None and list(lds) == [12, 12]


# ---------------------------------------------------------------- 3 the call sites, by ast
C_TO_TORCH = {"float": torch.float32, "double": torch.float64, "int32_t": torch.int32, "uint32_t": torch.int32,
              "int64_t": torch.int64, "uint8_t": torch.uint8}

# L.call sites whose arguments do not resolve positionally, each with its reason:
# (module, function, entry point or None where the name itself is computed)
INDIRECT = {
    ("pipeline.py", "weighted_sum", None): "one body for mmb_sif_wavg and mmb_sif_wavg_tt: `*tab` carries the "
                                           "table and, for a 16-bit table, its type",
    ("pipeline.py", "refresh", "mmb_mm2_prepare"): "the generators' parameters as four arrays of pointers "
                                                   "(arr(i)), every entry through L.ptr(.., L.F32)",
    ("pipeline.py", "mm2_stream", "mmb_mm2_stream_split"): "`*text, *frames, *tail`: the argument groups the "
                                                           "three stream entry points share",
    ("pipeline.py", "mm2_stream", "mmb_mm2_stream_tt"): "`*frames, *tail` (as above)",
    ("pipeline.py", "mm2_stream", "mmb_mm2_stream_ft"): "`*gathered, *frames, *tail` (as above)",
    ("pipeline.py", "mm2_stream", "mmb_mm2_stream"): "`*text, *frames, *tail` (as above)",
    ("pipeline.py", "_stream_project", None): "one body for the four fused entry points: optional text cache, "
                                              "the entry's own text arguments, optional frame type",
    ("sentiment_model.py", "run", "mmb_mlp_train"): "`*vargs`: the validation operands, or nulls without an "
                                                    "in-kernel validation",
    ("latent.py", "forward", "mmb_gauss_loglik_strided"): "host arrays of pointers and strides from _ptr_array / "
                                                          "_rows_array (checked per entry)",
    ("latent.py", "backward", "mmb_gauss_backward_strided"): "host arrays of pointers and strides (as above)",
}


def _modules():
    for name in sorted(os.listdir(PKG)):
        if name.endswith(".py"):
            yield name, ast.parse(open(os.path.join(PKG, name)).read(), name)


def _is_attr_call(node, obj, attr):
    return (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == attr
            and isinstance(node.func.value, ast.Name) and node.func.value.id == obj)


def _stated_dtype(node):
    """The dtype(s) an `L.ptr(x, L.NAME)` states, as a tuple; None if it is not of that form."""
    if not _is_attr_call(node, "L", "ptr") or len(node.args) != 2:
        return None
    d = node.args[1]
    if not (isinstance(d, ast.Attribute) and isinstance(d.value, ast.Name) and d.value.id in ("L", "torch")):
        return None
    v = getattr(L if d.value.id == "L" else torch, d.attr)
    return v if isinstance(v, tuple) else (v,)


def _ptr_exprs(node):
    """The L.ptr calls an argument may evaluate to (through `a if c else b`);
    None if some branch is neither an L.ptr call nor a literal None."""
    if isinstance(node, ast.IfExp):
        a, b = _ptr_exprs(node.body), _ptr_exprs(node.orelse)
        return None if a is None or b is None else a + b
    if isinstance(node, ast.Constant) and node.value is None:
        return []
    if _is_attr_call(node, "L", "ptr"):
        return [node]
    return None


def _call_sites():
    """(module, enclosing function, entry name or None, call node) of every L.call."""
    for mod, tree in _modules():
        for fn in ast.walk(tree):
            if not isinstance(fn, ast.FunctionDef):
                continue
            # (a call inside a nested function belongs to that function)
            inner = {id(c) for n in ast.walk(fn) if isinstance(n, ast.FunctionDef) and n is not fn
                     for c in ast.walk(n)}
            for node in ast.walk(fn):
                if id(node) in inner or not _is_attr_call(node, "L", "call"):
                    continue
                first = node.args[0]
                name = first.value if isinstance(first, ast.Constant) else None
                yield mod, fn.name, name, node


def test_every_ptr_states_a_dtype():
    n = 0
    for mod, tree in _modules():
        for node in ast.walk(tree):
            if _is_attr_call(node, "L", "ptr"):
                n += 1
                # (a helper that builds an array of pointers hands its own `dtype` argument on)
                assert len(node.args) == 2 and (_stated_dtype(node) is not None or isinstance(node.args[1], ast.Name)), \
                    f"{mod}:{node.lineno}: L.ptr without a stated dtype"
            # L.ptr handed on as a function (map(L.ptr, ...)) would state none
            if isinstance(node, ast.Call):
                for a in node.args:
                    assert not (isinstance(a, ast.Attribute) and a.attr == "ptr" and isinstance(a.value, ast.Name)
                                and a.value.id == "L"), f"{mod}:{node.lineno}: L.ptr passed as a function"
    assert n >= 100


def test_no_bare_data_ptr_reaches_the_library():
    """Outside mmb_lib, `.data_ptr()` appears only where an address is compared
    or tested (cache keys, alignment, aliasing), never as a call argument of
    L.call / L.query or inside a ctypes array."""
    for mod, tree in _modules():
        if mod == "mmb_lib.py":
            continue
        for node in ast.walk(tree):
            if not isinstance(node, ast.Call):
                continue
            to_lib = _is_attr_call(node, "L", "call") or _is_attr_call(node, "L", "query")
            ctypes_array = isinstance(node.func, ast.BinOp) or (
                isinstance(node.func, ast.Name) and node.func.id == "ctypes_ptr_array")
            if to_lib or ctypes_array:
                for sub in ast.walk(node):
                    assert not (isinstance(sub, ast.Attribute) and sub.attr == "data_ptr"), \
                        f"{mod}:{sub.lineno}: a bare data_ptr() handed to the library"


def test_stated_dtypes_match_the_header():
    protos = prototypes()
    resolved, unresolved = 0, set()
    for mod, fn, name, call in _call_sites():
        args = call.args[1:]
        if name is None or any(isinstance(a, ast.Starred) for a in args):
            unresolved.add((mod, fn, name))
            continue
        params = protos[name]
        assert len(args) == len(params), f"{mod}:{call.lineno}: {name} takes {len(params)} arguments"
        site_ok = True
        for a, (ctype, pname) in zip(args, params):
            if "*" not in ctype or pname.startswith("host_"):
                assert _ptr_exprs(a) in (None, []), f"{mod}:{call.lineno}: {name}({pname}) is no pointer"
                continue
            ptrs = _ptr_exprs(a)
            if ptrs is None:
                site_ok = False
                continue
            pointee = ctype.rstrip("*").strip()
            for p in ptrs:
                stated = _stated_dtype(p)
                assert stated is not None, f"{mod}:{p.lineno}"
                if pointee == "void":
                    continue
                assert stated == (C_TO_TORCH[pointee],), \
                    f"{mod}:{p.lineno}: {name}({pname}) is {ctype}, the mirror states {stated}"
        if site_ok:
            resolved += 1
        else:
            unresolved.add((mod, fn, name))
    assert unresolved == set(INDIRECT), (unresolved - set(INDIRECT), set(INDIRECT) - unresolved)
    assert resolved >= 30


def test_header_prototypes_parse():
    protos = prototypes()
    assert set(protos) == set(L.SIGNATURES)
    for name, (res, argtypes) in L.SIGNATURES.items():
        assert len(protos[name]) == len(argtypes), name
    assert protos["mmb_seq2weight"][:3] == [("int32_t*", "seq"), ("uint8_t*", "sel"), ("int64_t", "n")]
    assert ("float* const*", "mu") in protos["mmb_gauss_loglik_strided"]
    assert ("void*", "table") in protos["mmb_sif_wavg_tt"]
