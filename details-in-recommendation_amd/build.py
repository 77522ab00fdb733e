"""build.py -- compile libdir_hip.so (HIP kernels + C ABI) for gfx950, in-tree.

One hipcc invocation per translation unit (objects cached under csrc/_build by mtime), then one link.
The .so is git-ignored but travels with the gpurun snapshot.  No torch headers are involved: the
library is plain HIP behind the C ABI of include/dir_hip.h.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
BUILD = os.path.join(CSRC, "_build")
LIB = os.path.join(HERE, "libdir_hip.so")
SOURCES = ["capi.cpp", "embedding_bag.hip", "linear_cross.hip", "ids.hip", "cross.hip", "shard_bags.hip", "shard_linear.hip", "din.hip", "din_wave.hip", "din_pack.hip", "din_bwd_rows.hip", "din_rows_train.hip", "cin.hip", "cin_bf3.hip", "cin_dw_bf3.hip", "cin_dw_sym_bf3.hip", "cin_pool.hip", "cin_pooled.hip", "cin_bwd.hip", "backward.hip", "rows_scatter.hip", "radix_sort.hip", "dense.hip", "dense_bf3.hip", "tower_bf3.hip", "tower_cs.hip", "dense_dw_bf3.hip", "head_bwd.hip", "bn_train.hip", "dropout.hip", "rank_metrics.hip", "mf.hip", "diag.hip"]
# per-file flags: cin_bwd's epilogues read the MFMA results on the VALU, so keep them in VGPRs (no v_accvgpr_read)
NO_PACKED_FP32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
EXTRA_FLAGS = {"cin_bwd.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               # kernels that may share a SIMD with a bf16-MFMA kernel of another stream (the sharded lookup beside the CIN): no packed fp32
               # VALU instructions either, so that none of them can be the victim of the hazard described in isa_check.py
               "embedding_bag.hip": NO_PACKED_FP32,
               "shard_bags.hip": NO_PACKED_FP32,
               "shard_linear.hip": NO_PACKED_FP32,
               "backward.hip": NO_PACKED_FP32,
               "rows_scatter.hip": NO_PACKED_FP32,       # (the sharded backward's requester side; the same run sums as backward.hip)
               # cin_bf3 applies the field factor to the MFMA results on the VALU: keep them in VGPRs (no v_accvgpr_read); a packed fp32
               # VALU instruction beside bf16 MFMAs costs more than the two scalar ones it replaces
               "cin_bf3.hip": ["-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "dense_bf3.hip": ["-fno-slp-vectorize"],
               # tower_bf3's k loop must be unrolled completely (register arrays need static indices): 13 x 26 x 12 MFMAs exceed the default
               # full-unroll thresholds, and a rolled loop sends the activations to scratch
               "tower_bf3.hip": ["-fno-slp-vectorize", "-mllvm", "-unroll-threshold=1000000", "-mllvm", "-unroll-max-count=64",
                                 "-mllvm", "-unroll-full-max-count=64"],
               "cin_dw_bf3.hip": ["-fno-slp-vectorize"],
               "cin_dw_sym_bf3.hip": ["-fno-slp-vectorize"],
               "dense_dw_bf3.hip": ["-fno-slp-vectorize"],
               # din_wave's queue ticket is ONE lane's atomic whose result is consumed a sample later; the atomic optimizer would rewrite
               # it as a wave reduction + immediate s_waitcnt / readfirstlane, putting the round trip back on the critical path
               # ... and NO packed fp32 VALU instructions beside its 16x16x32 bf16 MFMAs (a gfx950 hazard: see the file's header and
               # tools/pk_mfma_probe.hip); the host pass prints "not a recognized feature" for the flag and ignores it
               "din_wave.hip": ["-mllvm", "-amdgpu-atomic-optimizer-strategy=None"] + NO_PACKED_FP32,
               "din_pack.hip": NO_PACKED_FP32,
               "cin_pooled.hip": NO_PACKED_FP32,
               "tower_cs.hip": NO_PACKED_FP32,
               "dropout.hip": NO_PACKED_FP32,             # (elementwise, on the training stream beside the other streams' bf16-MFMA kernels)
               "rank_metrics.hip": NO_PACKED_FP32,        # (evaluation beside a training or serving stream's bf16-MFMA kernels)
               "mf.hip": NO_PACKED_FP32,                  # (score / sampler streams beside another stream's bf16-MFMA kernels)
               "din_bwd_rows.hip": ["-mllvm", "-amdgpu-atomic-optimizer-strategy=None"] + NO_PACKED_FP32}
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
         "-Wall", "-Wno-unused-function"]
# DIR_DEVELOPMENT=1 python build.py --force: a build whose library honours the development A/B switches read from the environment
# (DIR_RS_DBG timing masks -- results are WRONG under them --, DIR_SORT, DIR_ADA_STAGE_MIN, DIR_BUCKET_EPT / _NT ...; csrc/common.hpp: dev_env;
# INTEGRATION.md lists them) and holds the kernel instantiations only they select.  The production build ignores them, compiles none of
# those kernels and refuses to sort when DIR_RS_DBG is set.
if os.environ.get("DIR_DEVELOPMENT") == "1":
    FLAGS.append("-DDIR_DEVELOPMENT")
# DIR_ABLATE="cin_bf3.hip:CIN_ABL=1": one timing-ablation macro for one translation unit (development; results are WRONG under most of them)
# DIR_NO_PK="a.hip,b.hip": those translation units without packed fp32 VALU instructions (development A/B)
for _f in filter(None, os.environ.get("DIR_NO_PK", "").split(",")):
    EXTRA_FLAGS[_f] = EXTRA_FLAGS.get(_f, []) + NO_PACKED_FP32
if os.environ.get("DIR_ABLATE"):
    _f, _m = os.environ["DIR_ABLATE"].split(":", 1)
    EXTRA_FLAGS[_f] = EXTRA_FLAGS.get(_f, []) + (NO_PACKED_FP32 if _m == "NO_PACKED_FP32" else ["-D" + d for d in _m.split(",")])


def _deps_mtime():
    hdrs = [os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".hpp")] + [os.path.join(HERE, "..", "include", "dir_hip.h")]
    return max(os.path.getmtime(h) for h in hdrs)


def _compile(src):
    s = os.path.join(CSRC, src)
    o = os.path.join(BUILD, os.path.splitext(src)[0] + ".o")
    if os.path.exists(o) and os.path.getmtime(o) >= max(os.path.getmtime(s), _deps_mtime()):
        return o
    cmd = [HIPCC] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-c", s, "-o", o]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (src, " ".join(cmd), r.stderr))
    err = "\n".join(l for l in r.stderr.split("\n") if "is not a recognized feature for this target" not in l)     # the host pass of NO_PACKED_FP32
    if err.strip():
        sys.stderr.write(err)
    return o


def _isa_check(objs):
    """isa_check.py over every object that changed since it was last checked (a stamp file beside the object)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("dir_isa_check", os.path.join(HERE, "isa_check.py"))
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    todo = [o for o in objs if not os.path.exists(o + ".isa_ok") or os.path.getmtime(o + ".isa_ok") < os.path.getmtime(o)]
    errors, exposed = isa.check(todo)
    if errors:
        raise RuntimeError("gfx950 hazard: packed fp32 VALU (op_sel high -> low) inside a kernel that issues 16x16x32 MFMAs (isa_check.py):\n" +
                           "\n".join("  %s: %s (%d x, e.g. %s)" % e for e in errors))
    for o, f, n in exposed:
        sys.stderr.write("isa_check: %s: %s holds %d packed fp32 instructions that a co-resident bf16-MFMA kernel can corrupt\n" % (o, f[:80], n))
    for o in todo:
        open(o + ".isa_ok", "w").close()


def build(force=False, jobs=None):
    os.makedirs(BUILD, exist_ok=True)
    if force:
        for f in os.listdir(BUILD):
            os.remove(os.path.join(BUILD, f))
    # MAX_JOBS (the usual cap of extension builds) wins over the machine's CPU count, which may be far more than this process may use
    jobs = jobs or int(os.environ.get("MAX_JOBS") or 0) or min(len(SOURCES), max(1, (os.cpu_count() or 2) // 2))
    with ThreadPoolExecutor(jobs) as ex:
        objs = list(ex.map(_compile, SOURCES))
    _isa_check(objs)
    if (not os.path.exists(LIB)) or any(os.path.getmtime(o) > os.path.getmtime(LIB) for o in objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n%s" % r.stderr)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
