"""The C ABI as the CPU tests read it: the entry points include/mmb.h declares
and the parameter names of the entry points whose argument tables the tests
walk (tests/test_lib_abi.py, tests/test_narrow_frames16_cases.py,
tests/test_split_frames16_cases.py).  Plain helper module: no test is
collected from it.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmb.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mmb_[a-z0-9_]+)\s*\(", src)))


def prototypes():
    """name -> [(C type, parameter name), ...] of every entry point the header
    declares, the type with `const` dropped and its `*`s kept ("float*",
    "void* const*", "int64_t")."""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, body in re.findall(r"\b(mmb_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        params = []
        for p in (q.strip() for q in body.split(",")):
            if p == "void" or not p:
                continue
            m = re.fullmatch(r"(.*?)(\w+)", p, flags=re.S)
            ctype = " ".join(m.group(1).split())
            ctype = re.sub(r"\s*\*\s*", "*", re.sub(r"^const ", "", ctype)).replace("*const*", "* const*")
            params.append((ctype, m.group(2)))
        out[name] = params
    return out


STREAM = ("ids table v wtab32 text_dense emb_dense w_dense audio visual n t d a vd num_out s_out "
          "s_half aux_out flag colmax colmax_ws").split()
ENTRY_ARGS = {
    "mmb_sif_wavg": "table v d ids n l w wtab32 x_out num_out cnt_out flag stream".split(),
    "mmb_mm2_stream": STREAM + ["stream"],
    "mmb_mm2_stream_split": STREAM + "parts ws ws_bytes stream".split(),
    "mmb_mm2_stream_project": ("ids table v wtab32 text_dense w_dense audio visual n t d a vd wpieces c0 "
                               "num_out aux_out mmb2_out flag colmax colmax_ws stream").split(),
    "mmb_mm2_stream_project_narrow": ("ids table v wtab32 text_cache audio visual n t d a vd wpieces c0 "
                                      "num_out aux_out mmb2_out flag colmax colmax_ws stream").split(),
    "mmb_mm2_project_x3": "s_split num aux wsplit ldw c0 n k d out stream".split(),
    "mmb_mm2_project_x3_rmpc": "s_split num aux wsplit ldw c0 n k d out pc sif_out stream".split(),
    "mmb_mm2_project_x3_split": ("s_split num aux wsplit ldw c0 n k d out pc sif_out slices ws ws_bytes "
                                 "stream").split(),
    "mmb_layer_norm_backward": "dy x mean rstd gamma n d dx dgamma dbeta stream".split(),
    "mmb_mm2_project": "s num aux wm ldw c0 n k d out stream".split(),
    "mmb_colmax": "x n d colmax accumulate stream".split(),
    "mmb_mlp_forward": "latents idx b d h o w1 b1 w2 b2 y_out stream".split(),
    "mmb_mlp_eval": "latents labels perm n batch d h o w1 b1 w2 b2 batch_loss pred_out stream".split(),
    "mmb_mlp_forward_train": "x b d h o w1 b1 w2 b2 y_out hid_out stream".split(),
    "mmb_mlp_backward": "x hid b d h o w1 w2 dy dh_ws dx dw1 db1 dw2 db2 stream".split(),
    "mmb_word_logprob_forward": ("latents b d wn v ids table sent_dense l w mask a want_grad ws lp state gsum "
                                 "cos_out stream").split(),
    "mmb_word_logprob_backward": ("latents b d v ids table sent_dense l w mask a state gsum cosv dlp dlat "
                                  "stream").split(),
}
