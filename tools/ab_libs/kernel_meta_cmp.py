"""Do two builds of libmmb.so hold the same code for the kernels they share?

    python tools/ab_libs/kernel_meta_cmp.py OLD/libmmb.so NEW/libmmb.so

Reads the gfx950 code objects of both libraries (llvm-objdump --offloading,
llvm-readelf --notes / --symbols; no GPU) and compares, for every kernel of
OLD, the code-object metadata of its counterpart in NEW -- VGPR / SGPR / AGPR
counts, spills, scratch and LDS bytes -- and the size of its code.  A kernel
whose template list only grew a defaulted trailing parameter counts as the
same kernel (RENAMES: the split stream's and the text cache's kernels gained
the word table's element type).  Exit status 1 when a kernel of OLD is
missing from NEW or differs."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
KEYS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size")

# NEW's mangled name -> OLD's, for kernels that became templates on the word
# table's element type (float: the kernel OLD had)
RENAMES = (
    (re.compile(r"(utt_split_part_kernelILi\d+ELi\d+ELi\d+ELi\d+ELi\d+E(?:f|DF16_|NS_6bf16_tE))fE"), r"\1E"),
    (re.compile(r"23utt_split_finish_kernelIfEEvNS_"), "23utt_split_finish_kernelENS_"),
    (re.compile(r"21mm2_text_table_kernelIfEEvPKT_iPKfiPf"), "21mm2_text_table_kernelEPKfiS1_iPf"),
)


def old_name(name: str) -> str:
    for pat, rep in RENAMES:
        name = pat.sub(rep, name)
    return name


def kernels(lib: str) -> dict:
    """{kernel: {metadata key: value, "code_bytes": n}} over every gfx950 code object of lib"""
    tmp = tempfile.mkdtemp()
    try:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp, check=True,
                       capture_output=True)
        out = {}
        for co in glob.glob(os.path.join(tmp, "lib.so.*gfx950*")):
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True,
                                   text=True).stdout
            # a kernel's entry starts at its (alphabetically first) .agpr_count key
            for entry in re.split(r"\n  - (?=\.agpr_count:)", notes)[1:]:
                entry = entry.split("\namdhsa.target:")[0]
                name = re.search(r"\n    \.name:\s+(\S+)", entry).group(1)
                out[name] = {k: int(re.search(r"(?:^|\n    )" + re.escape(k) + r":\s+(\d+)", entry).group(1))
                             for k in KEYS}
            syms = subprocess.run([f"{LLVM}/llvm-readelf", "--symbols", "-W", co], check=True,
                                  capture_output=True, text=True).stdout
            for line in syms.splitlines():
                p = line.split()
                if len(p) >= 8 and p[3] == "FUNC" and p[7] in out:
                    out[p[7]]["code_bytes"] = int(p[2])
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main(old_lib: str, new_lib: str) -> int:
    old, new = kernels(old_lib), kernels(new_lib)
    by_old = {old_name(k): k for k in new}
    missing = sorted(k for k in old if k not in by_old)
    differ = sorted(k for k in old if k in by_old and new[by_old[k]] != old[k])
    renamed = sorted(k for k in old if k in by_old and by_old[k] != k)
    added = sorted(k for k in new if old_name(k) not in old)
    print(f"kernels: {len(old)} old, {len(new)} new; {len(renamed)} renamed, {len(added)} added")
    for k in missing:
        print(f"MISSING {k}")
    for k in differ:
        print(f"DIFFERS {k}\n  old {old[k]}\n  new {new[by_old[k]]}")
    for k in added:
        print(f"added {k} {new[k]}")
    print(f"{len(missing)} missing, {len(differ)} differ" if missing or differ
          else "every kernel of the old build has the same metadata and code size in the new one")
    return 1 if missing or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
