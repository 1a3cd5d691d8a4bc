"""CPU: the C-ABI library loads and exports every symbol include/mmb.h declares.

No compute calls here (no GPU in the build container) except the host-only
RNG helper, which is checked bit for bit against numpy's legacy RandomState.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import mmb_lib
from abi_cases import ENTRY_ARGS, ROOT, declared_functions


def test_header_declares_entry_points():
    names = declared_functions()
    assert "mmb_sif_wavg" in names and "mmb_pc_solve" in names and "mmb_mlp_train" in names
    assert len(names) >= 19


def test_library_exports_every_declared_symbol():
    lib = mmb_lib.load()
    for name in declared_functions():
        assert hasattr(lib, name), f"{name} declared in mmb.h but not exported"


def test_ctypes_signatures_cover_header():
    assert set(declared_functions()) == set(mmb_lib.SIGNATURES)


def test_exports_are_c_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", mmb_lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (mmb_\w+)", out))
    assert set(declared_functions()) <= exported  # unmangled extern "C"


def test_product_library_reads_no_knobs():
    """The product library carries only the default kernels: no getenv, no
    MMB_* knob string, no timing-only DIAG build (those live in the tools
    build libmmb_diag.so, `make diag`)."""
    path = os.path.join(ROOT, "multimodal-baselines_amd", "libmmb.so")
    blob = open(path, "rb").read()
    assert b"DIAG" not in blob
    assert re.search(rb"MMB_[A-Z_]{3,}", blob) is None
    undef = subprocess.run(["nm", "-D", "--undefined-only", path], capture_output=True, text=True,
                           check=True).stdout
    assert "getenv" not in undef


def test_product_sources_carry_no_tools_code():
    """The product kernel sources hold only what libmmb.so runs (r06): no
    environment reads and no MMB_DIAG blocks -- the tools build's variants,
    knobs and probes live in tools/diag/ and plug into named MMB_HOOK_*
    points whose product defaults are compiled here.  Nor any build-time
    switch: the constants once set with -D by clone scripts are constexpr."""
    macros = ("MMB_SPLIT_TEXT_X", "MMB_SPLIT_TU", "MMB_SPLIT_FU", "NF_UNR", "NF_HU", "NF_ABL",
              "NF_GA", "NF_GV", "NF_WAVES", "MMB_SQ_PER_WG")
    csrc = os.path.join(ROOT, "multimodal-baselines_amd", "csrc")
    srcs = [f for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".cpp"))]
    assert "sif_kernels.hip" in srcs and "pc_kernels.hip" in srcs
    assert "fused_kernels.hip" in srcs and "narrow_fused_kernels.hip" in srcs
    assert "gram_kernels.hip" in srcs and "pc_remove_kernels.hip" in srcs and "mmb_pc.h" in srcs
    for f in srcs:
        text = open(os.path.join(csrc, f)).read()
        assert "getenv" not in text, f
        assert "MMB_DIAG" not in text, f
        for m in macros:
            assert m not in text, (f, m)
    # the tails the tools build includes exist; the product's target is empty
    for tail in ("sif_tail.inc", "fused_tail.inc", "narrow_fused_tail.inc", "pc_tail.inc", "mm2_tail.inc",
                 "gram_tail.inc", "pc_remove_tail.inc", "diag_hooks.h"):
        assert os.path.exists(os.path.join(ROOT, "tools", "diag", tail)), tail
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "mmb_no_tools.h")).read())
    assert code.strip() == ""


def test_pc_solve_workspace_layout():
    """control words | tiles | G2 | z0, laid out once (SolveWs, csrc/pc_kernels.hip):
    16 + 2 (d / 16 + 1) 4096 + 8 d^2 + 128 d bytes; a negative d sizes as d = 0."""
    for d in (0, 1, 15, 16, 17, 300, 320):
        assert mmb_lib.query("mmb_pc_solve_mc_ws_bytes", d) == \
            16 + 2 * (d // 16 + 1) * 4096 + 8 * d * d + 128 * d, d
    assert mmb_lib.query("mmb_pc_solve_mc_ws_bytes", 0) == 8_208
    assert mmb_lib.query("mmb_pc_solve_mc_ws_bytes", 16) == 20_496
    assert mmb_lib.query("mmb_pc_solve_mc_ws_bytes", 300) == 914_064
    assert mmb_lib.query("mmb_pc_solve_mc_ws_bytes", 320) == 1_032_208
    for d in (-1, -300):
        assert mmb_lib.query("mmb_pc_solve_mc_ws_bytes", d) == 8_208, d


def test_gram_workspace_sizes_are_pinned():
    """mmb_gram_workspace_bytes (csrc/gram_kernels.hip: the largest of its four
    planners' partials) as the library returned it before the Gram sources
    were split out of pc_kernels.hip."""
    pinned = {(1, 4): 32_768, (1284, 300): 9_338_880, (4097, 300): 24_903_680,
              (1_000_000, 300): 62_914_560, (1000, 301): 6_225_920, (1000, 512): 17_301_504}
    for (n, d), want in pinned.items():
        assert mmb_lib.query("mmb_gram_workspace_bytes", n, d) == want, (n, d)


def test_library_carries_gfx950_code_objects():
    data = open(mmb_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in data


def test_version_and_shape_helpers():
    assert mmb_lib.query("mmb_version") >= 100
    assert mmb_lib.query("mmb_mm2_k", 300, 300, 300) == 1824
    assert mmb_lib.query("mmb_mm2_k", 300, 76, 48) == 864
    assert mmb_lib.query("mmb_mm2_ldw", 300) == 320
    assert mmb_lib.query("mmb_gram_workspace_bytes", 1_000_000, 300) > 0
    # arrival counter + abort word, then 2 x 4 hidden tiles x 32 rows x 16 outputs of f32 shares
    assert mmb_lib.query("mmb_mlp_workspace_bytes", 300, 100) == 16 + 4 * 2 * 4 * 32 * 16


@pytest.mark.parametrize("seed,rows,k", [(0, 300, 11), (0, 64, 11), (0, 1, 12), (7, 1000, 3)])
def test_host_randn_matches_numpy_randomstate(seed, rows, k):
    got = mmb_lib.host_randn(seed, rows * k)
    ref = np.random.RandomState(seed).normal(size=(rows, k)).ravel()
    assert np.array_equal(got, ref)


def test_invalid_arguments_rejected_without_gpu():
    # argument validation happens before any launch
    with pytest.raises(mmb_lib.MMBError):
        mmb_lib.call("mmb_pc_solve", None, 300, None, 11, 1, 7, 0, None, None)
    with pytest.raises(mmb_lib.MMBError):
        mmb_lib.call("mmb_host_randn", 0, -1, None)


# ---- the same for the stream and x3 projection entry points, as a table: ----
# ---- argument checks and empty calls that return before any device call  ----
# Stand-ins for device pointers: 16-byte aligned, never dereferenced (every
# row below returns before a launch or a device query).
P = 0x7F0000001000
KCMAX_ROWS = 8192  # rows of the column-bound workspace (mmb_mm2_colmax_ws_bytes(d) // (4 d))

# a valid gathered-text call of each kind (n > 0: it would go on to launch)
GATHER = dict(ids=P, table=P, v=1000, wtab32=P, text_dense=None, emb_dense=None, w_dense=None, audio=P,
              visual=P, n=100, t=40, d=300, a=300, vd=300, num_out=P, s_out=P, s_half=1, aux_out=P,
              flag=None, colmax=None, colmax_ws=None, stream=None)
BASE = {
    "mmb_sif_wavg": dict(table=P, v=1000, d=300, ids=P, n=100, l=40, w=None, wtab32=P, x_out=P,
                         num_out=None, cnt_out=None, flag=None, stream=None),
    "mmb_mm2_stream": GATHER,
    # parts > 0: parts = 0 asks the device for its CU count
    "mmb_mm2_stream_split": dict(GATHER, parts=2, ws=P, ws_bytes=1 << 40),
    "mmb_mm2_stream_project": dict(GATHER, wpieces=P, c0=P, mmb2_out=P),
    "mmb_mm2_stream_project_narrow": dict(GATHER, v=3016, t=20, a=76, vd=48, text_cache=P, wpieces=P, c0=P,
                                          mmb2_out=P),
}
X3 = dict(s_split=P, num=P, aux=P, wsplit=P, ldw=320, c0=P, n=100, k=1824, d=300, out=P, pc=None,
          sif_out=None, slices=2, ws=P, ws_bytes=1 << 40, stream=None)  # slices = 0 asks the device
for _name in ("mmb_mm2_project_x3", "mmb_mm2_project_x3_rmpc", "mmb_mm2_project_x3_split"):
    BASE[_name] = X3
BASE["mmb_layer_norm_backward"] = dict(dy=P, x=P, mean=P, rstd=P, gamma=P, n=100, d=300, dx=P, dgamma=P, dbeta=P,
                                       stream=None)
MLP = dict(latents=P, x=P, hid=P, idx=None, labels=P, perm=None, b=100, n=100, batch=32, d=300, h=100, o=1, w1=P,
           b1=P, w2=P, b2=P, y_out=P, hid_out=P, batch_loss=P, pred_out=P, dy=P, dh_ws=P, dx=P, dw1=P, db1=P,
           dw2=P, db2=P, stream=None)
WORD = dict(latents=P, b=64, d=300, wn=P, v=3016, ids=P, table=P, sent_dense=None, l=20, w=P, mask=P, a=1e-3,
            want_grad=1, ws=P, lp=P, state=P, gsum=P, cos_out=P, cosv=P, dlp=P, dlat=P, stream=None)
BASE.update({"mmb_mm2_project": dict(X3, s=P, wm=P), "mmb_colmax": dict(x=P, n=100, d=300, colmax=P, accumulate=0,
                                                                      stream=None),
             "mmb_mlp_forward": MLP, "mmb_mlp_eval": MLP, "mmb_mlp_forward_train": MLP, "mmb_mlp_backward": MLP,
             "mmb_word_logprob_forward": WORD, "mmb_word_logprob_backward": WORD})
DENSE = dict(ids=None, table=None, v=0, wtab32=None, text_dense=P, emb_dense=P, w_dense=P)
BOUNDS = dict(colmax=P, colmax_ws=P)
EINVAL, OK = -1, 0


def _split_ws_bytes(**kw):
    a = dict(GATHER, parts=2, **kw)
    return mmb_lib.query("mmb_mm2_stream_split_ws_bytes", a["n"], a["t"], a["d"], a["a"], a["vd"], a["parts"])


CASES = [
    ("mmb_mm2_stream", "scalar D 321", dict(d=321), EINVAL),
    ("mmb_mm2_stream", "scalar A 321", dict(a=321), EINVAL),
    ("mmb_mm2_stream", "scalar Vd 321", dict(vd=321), EINVAL),
    ("mmb_mm2_stream", "bounds without workspace", dict(colmax=P), EINVAL),
    ("mmb_mm2_stream", "bounds at D 644", dict(BOUNDS, d=644), EINVAL),
    ("mmb_mm2_stream", "ids without table", dict(table=None), EINVAL),
    ("mmb_mm2_stream", "dense text without emb_dense", dict(DENSE, emb_dense=None), EINVAL),
    ("mmb_mm2_stream", "s_half 2", dict(s_half=2), EINVAL),
    ("mmb_mm2_stream_split", "bounds with n past the workspace rows", dict(BOUNDS, n=KCMAX_ROWS + 1), EINVAL),
    ("mmb_mm2_stream_split", "workspace one byte short", lambda: dict(ws_bytes=_split_ws_bytes() - 1), EINVAL),
    ("mmb_mm2_stream_split", "past the finish kernel's columns", dict(d=512), EINVAL),
    ("mmb_mm2_stream_split", "parts -1", dict(parts=-1), EINVAL),
    ("mmb_mm2_stream_project", "audio misaligned by 4 bytes", dict(audio=P + 4), EINVAL),
    ("mmb_mm2_stream_project", "D 252", dict(d=252), EINVAL),
    ("mmb_mm2_stream_project", "D 320", dict(d=320), EINVAL),
    ("mmb_mm2_stream_project", "A 322", dict(a=322), EINVAL),
    ("mmb_mm2_stream_project", "missing wpieces", dict(wpieces=None), EINVAL),
    ("mmb_mm2_stream_project_narrow", "V 16385", dict(v=16385), EINVAL),
    ("mmb_mm2_stream_project_narrow", "A 132", dict(a=132), EINVAL),
    ("mmb_mm2_stream_project_narrow", "D 256", dict(d=256), EINVAL),
    ("mmb_mm2_stream_project_narrow", "missing text_cache", dict(text_cache=None), EINVAL),
]
for _name in ("mmb_mm2_project_x3", "mmb_mm2_project_x3_rmpc", "mmb_mm2_project_x3_split"):
    CASES += [(_name, "k 100", dict(k=100), EINVAL),
              (_name, "ldw 384", dict(ldw=384), EINVAL),
              (_name, "misaligned s_split", dict(s_split=P + 8), EINVAL)]
    if _name != "mmb_mm2_project_x3":
        CASES.append((_name, "pc without sif_out", dict(pc=P), EINVAL))
# the empty call without bounds: MMB_OK, nothing enqueued (the split one before
# its workspace is looked at or its plan asks the device)
CASES += [(name, "n 0", dict(n=0), OK) for name in ("mmb_sif_wavg", "mmb_mm2_stream", "mmb_mm2_stream_project",
                                                    "mmb_mm2_stream_project_narrow")]
CASES.append(("mmb_mm2_stream_split", "n 0, no workspace", dict(n=0, parts=0, ws=None, ws_bytes=0), OK))
# the host guards of 32-bit grids and row indices, on their refused side (the
# accepted side of each would go on to launch: tests/test_gpu_large.py where a
# device can hold it).  The workspaces are claimed large enough, so the size
# check before each guard passes and the guard itself answers.
HUGE_WS = 1 << 62
CASES += [
    # rows are 32-bit in the narrow fused kernel: n < 2^31 - 32 (one batch of rows past the last)
    ("mmb_mm2_stream_project_narrow", "n 2^31 - 32", dict(n=2 ** 31 - 32), EINVAL),
    # t = 40 in 2 parts: Pt + 2 Pf = 6 workgroups per row; the grid n (Pt + 2 Pf) <= 2^31 - 1
    ("mmb_mm2_stream_split", "grid past 2^31 - 1", dict(n=(2 ** 31 - 1) // 6 + 1, ws_bytes=HUGE_WS), EINVAL),
    # 128-row tiles in 2 slices: tiles nsl <= 2^31 - 1
    ("mmb_mm2_project_x3_split", "grid past 2^31 - 1", dict(n=128 * 2 ** 30 + 1, ws_bytes=HUGE_WS), EINVAL),
    # LayerNorm backward: n <= 2^33, and rb + cb < 2^31 blocks (rb = ceil(n / 4) row blocks, cb =
    # ceil(d / 64) column blocks where dgamma or dbeta is asked for)
    ("mmb_layer_norm_backward", "n 2^33 + 1", dict(n=2 ** 33 + 1), EINVAL),
    ("mmb_layer_norm_backward", "rb + cb = 2^31 + 4", dict(n=4 * (2 ** 31 - 1)), EINVAL),
    ("mmb_layer_norm_backward", "rb = 2^31", dict(n=2 ** 33, dgamma=None, dbeta=None), EINVAL),
    ("mmb_layer_norm_backward", "n 0, no column sums", dict(n=0, dgamma=None, dbeta=None), OK),
    # kMaxGridX (csrc/mmb_common.h): a workgroup per row, or per block of rows, and no grid-stride
    # loop -- 2^31 workgroups are refused where the cast to the launch's grid would wrap
    ("mmb_mm2_stream", "workgroup route, fp16 s, n 2^31", dict(t=65, n=2 ** 31), EINVAL),
    ("mmb_mm2_project", "2^31 tiles of 64 rows", dict(n=64 * 2 ** 31), EINVAL),
    ("mmb_mm2_project_x3", "2^31 tiles of 128 rows", dict(n=128 * 2 ** 31), EINVAL),
    ("mmb_colmax", "2^31 blocks of 256 rows", dict(n=256 * 2 ** 31), EINVAL),
    ("mmb_mlp_forward", "2^31 batches of 32 rows", dict(b=32 * 2 ** 31), EINVAL),
    ("mmb_mlp_eval", "2^31 batches", dict(n=2 ** 31, batch=1), EINVAL),
    ("mmb_mlp_forward_train", "2^31 blocks of 8 rows", dict(b=8 * 2 ** 31), EINVAL),
    ("mmb_mlp_backward", "2^31 blocks of 2 rows", dict(b=2 * 2 ** 31), EINVAL),
    ("mmb_word_logprob_forward", "b 2^31", dict(b=2 ** 31), EINVAL),
    ("mmb_word_logprob_backward", "b 2^31", dict(b=2 ** 31), EINVAL),
]


def test_gauss_rows_past_the_grid_are_rejected_without_gpu():
    """mmb_gauss_loglik / _backward launch a workgroup per row and key: 2^31 rows are refused."""
    import ctypes

    arr = lambda t, *v: (t * len(v))(*v)
    head = [arr(ctypes.c_void_p, P, 0, 0), arr(ctypes.c_int, 4, 0, 0), None, 2 ** 31, 1, arr(ctypes.c_int, 1),
            arr(ctypes.c_void_p, P), arr(ctypes.c_void_p, P)]
    with pytest.raises(mmb_lib.MMBError, match=r"code -1 \(invalid argument\)"):
        mmb_lib.call("mmb_gauss_loglik", *head, P, None)
    with pytest.raises(mmb_lib.MMBError, match=r"code -1 \(invalid argument\)"):
        mmb_lib.call("mmb_gauss_backward", *head, P, arr(ctypes.c_void_p, P), arr(ctypes.c_void_p, P), None)
    with pytest.raises(mmb_lib.MMBError, match="2\\^31 - 1"):
        mmb_lib.check_grid("gauss_log_prob", 2 ** 31)
    mmb_lib.check_grid("colmax", 256 * (2 ** 31 - 1), 256)


def test_case_table_starts_from_valid_calls():
    """Every rejection row changes one thing of a call the library's own
    shape queries accept, so the rejection is the row's and not the base's."""
    g = GATHER
    assert mmb_lib.query("mmb_mm2_stream_project_supported", g["t"], g["d"], g["a"], g["vd"])
    nf = BASE["mmb_mm2_stream_project_narrow"]
    assert mmb_lib.query("mmb_mm2_stream_project_narrow_supported", nf["t"], nf["d"], nf["a"], nf["vd"], nf["v"])
    assert X3["ldw"] == mmb_lib.query("mmb_mm2_ldw", X3["d"])
    assert X3["k"] == mmb_lib.query("mmb_mm2_k", X3["d"], 300, 300)
    assert mmb_lib.query("mmb_mm2_colmax_ws_bytes", g["d"]) // (4 * g["d"]) == KCMAX_ROWS
    assert 0 < _split_ws_bytes() < BASE["mmb_mm2_stream_split"]["ws_bytes"]
    assert 0 < _split_ws_bytes(d=512) < BASE["mmb_mm2_stream_split"]["ws_bytes"]


@pytest.mark.parametrize("name,what,change,want", CASES, ids=[f"{c[0]}-{c[1]}".replace(" ", "_") for c in CASES])
def test_invalid_arguments_rejected_without_gpu_table(name, what, change, want):
    # argument validation, and the empty call, happen before any launch
    filled = dict(BASE[name], **(change() if callable(change) else change))
    args = [filled[k] for k in ENTRY_ARGS[name]]
    if want == OK:
        assert mmb_lib.call(name, *args) == 0
    else:
        with pytest.raises(mmb_lib.MMBError, match=r"code -1 \(invalid argument\)"):
            mmb_lib.call(name, *args)


def test_environment_cannot_redirect_the_product_library(tmp_path):
    """MMB_LIB_PATH (the round-3 A/B hook) no longer exists: a fresh process
    with it set to the tools build still loads libmmb.so; the tools build is
    reachable only through an explicit mmb_lib.load(path)."""
    import sys
    diag = os.path.join(ROOT, "tools", "diag", "libmmb_diag.so")
    code = ("import sys; sys.path.insert(0, %r); import mmb_lib; mmb_lib.load(); "
            "print(mmb_lib.loaded_path())" % os.path.join(ROOT, "multimodal-baselines_amd"))
    env = {**os.environ, "MMB_LIB_PATH": diag, "MMB_TOOLS_LIB": diag}
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                         check=True).stdout.strip().splitlines()[-1]
    assert out == os.path.join(ROOT, "multimodal-baselines_amd", "libmmb.so")
    src = open(os.path.join(ROOT, "multimodal-baselines_amd", "mmb_lib.py")).read()
    assert "os.environ" not in src and "getenv" not in src
    # nor does the step read options from the environment: its constructor
    # arguments are the only way to force a path
    src = open(os.path.join(ROOT, "multimodal-baselines_amd", "pipeline.py")).read()
    assert "os.environ" not in src and "getenv" not in src


def test_second_library_path_is_refused():
    lib = mmb_lib.load()
    assert mmb_lib.load() is lib
    with pytest.raises(mmb_lib.MMBError):
        mmb_lib.load(os.path.join(ROOT, "tools", "diag", "libmmb_diag.so"))
