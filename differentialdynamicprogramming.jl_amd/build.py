"""Builds libddp_amd.so (HIP, gfx950) in-tree:  python build.py [--force]

One hipcc invocation per translation unit (run in parallel), then a link step.  hipcc
cross-compiles for gfx950 without a GPU, so this also runs in the CPU-only build container.
"""
import concurrent.futures as cf
import hashlib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libddp_amd.so")
SOURCES = ["capi.hip", "back_pass.hip", "back_pass_dpp.hip", "back_pass_dppw.hip", "back_pass_row.hip", "back_pass_row_hi.hip", "back_pass_mid.hip", "back_pass_big.hip", "back_pass_gps_lane.hip", "back_pass_mfma.hip", "back_pass_mfma_lims.hip", "back_pass_mf2.hip", "back_pass_mf2_lims.hip", "back_pass_mx.hip", "back_pass_mxg.hip", "back_pass_mx2.hip", "back_pass_sh.hip", "back_pass_q4.hip", "back_pass_wide.hip",
           "forward_pass.hip", "forward_pass_dpp.hip", "forward_pass_row.hip", "forward_pass_pipe.hip", "forward_pass_big.hip", "forward_pass_wide.hip", "df.hip", "ilqg.hip", "kl.hip", "kl_wide.hip", "comm.hip", "boxqp_big.hip", "user_program.hip", "user_problem.hip", "sample.hip", "fit.hip", "gmm.hip", "expect.hip", "fit_wide.hip"]
HEADERS = ["ddp_internal.h", "boxqp_dev.h", "boxqp_rows.h", "staging.h", os.path.join("..", "..", "include", "ddp_amd.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Rpass-analysis=kernel-resource-usage", "-Wall", "-Wno-unused-function",
         "-Wno-unused-but-set-variable", "-Wno-unused-variable"]


# MFMA accumulators stay in the (unified) VGPR file: no v_accvgpr_read/write shuffles around every product
EXTRA_FLAGS = {"back_pass_mx.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "back_pass_mxg.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "back_pass_mx2.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "back_pass_sh.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "back_pass_mid.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "back_pass_q4.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "back_pass_mfma.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "back_pass_mf2.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "back_pass_mf2_lims.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "back_pass_wide.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "kl_wide.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "fit.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "fit_wide.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "gmm.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "expect.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"],
               "user_program.hip": ["-I", OBJ]}                  # the headers of PROGRAM_TEXTS, written to build/


EXTRA_DEPS = {"user_program.hip": ["user_program.h", "user_problem_kernels.h", "user_problem_wave_kernels.h", "user_autodiff.h", "user_constraints.h", "user_sample_kernels.h", "user_sample_wave_kernels.h", "user_fitted_kernels.h", "user_fitted_wave_kernels.h", "user_cost_fit_kernels.h", "philox.h", "wide_tile.h", "back_pass_wide_kernel.h"],
              "user_problem.hip": ["user_program.h", "user_problem_kernels.h", "user_constraints.h", "user_sample_kernels.h", "user_fitted_kernels.h", "user_cost_fit_kernels.h", "wide_tile.h", "back_pass_wide_kernel.h"], "sample.hip": ["philox.h"], "back_pass_mf2.hip": ["back_pass_mf2_kernel.h"], "back_pass_mf2_lims.hip": ["back_pass_mf2_kernel.h"], "back_pass_row_hi.hip": ["back_pass_row.hip"], "back_pass_mfma.hip": ["back_pass_mfma_kernel.h"], "back_pass_mfma_lims.hip": ["back_pass_mfma_kernel.h"],
              "back_pass_mx.hip": ["back_pass_mx_common.h"], "back_pass_mxg.hip": ["back_pass_mx_common.h"], "back_pass_mx2.hip": ["back_pass_mx_common.h"], "back_pass_sh.hip": ["back_pass_mx_common.h"],
              "ilqg.hip": ["ilqg_model.h", "carver.h"], "kl.hip": ["ilqg_model.h", "carver.h", "kl_workspace.h"], "forward_pass_dpp.hip": ["pend_math.h"], "back_pass_wide.hip": ["wide_tile.h", "back_pass_wide_kernel.h"], "kl_wide.hip": ["wide_tile.h"], "fit.hip": ["wide_tile.h"], "fit_wide.hip": ["wide_tile.h"], "gmm.hip": ["wide_tile.h", "philox.h"], "expect.hip": ["wide_tile.h"]}


# Headers of csrc/ as program text for hiprtc (user_program.hip): output file -> [(symbol, header)].  The kernels compiled at run time take
# the definitions the precompiled ones include, one definition for both compilers: ddp_user_back_pass2 factorises and solves with
# boxqp_dev.h, ddp_user_back_pass2_wave (DDP_USER_SECOND_ORDER_WAVE) is the step of back_pass_wide.hip, ddp_user_sample (DDP_USER_SAMPLE)
# and ddp_user_sample_wave (DDP_USER_SAMPLE_WAVE) draw their normals with the philox.h of sample.hip.
PROGRAM_TEXTS = {"boxqp_dev_text.h": [("kBoxqpDevText", "boxqp_dev.h")],
                 "wide_kernel_text.h": [("kWideTileText", "wide_tile.h"), ("kWideKernelText", "back_pass_wide_kernel.h")],
                 "philox_text.h": [("kPhiloxText", "philox.h")]}


def _program_texts():
    """PROGRAM_TEXTS -> build/.  A header's own #include lines and #pragma once are left out (hiprtc has no include path to them; ddp_rsqrt,
    the one thing boxqp_dev.h takes from ddp_internal.h, is part of the program text)."""
    for out, parts in PROGRAM_TEXTS.items():
        text = "// written by build.py from " + " and ".join("csrc/" + header for _, header in parts) + "\n"
        for name, header in parts:
            src = open(os.path.join(CSRC, header)).read()
            body = "".join(l for l in src.splitlines(True) if not l.startswith("#include") and not l.startswith("#pragma once"))
            assert ')DDPQ"' not in body
            text += "static const char *%s = R\"DDPQ(\n" % name + body + ")DDPQ\";\n"
        out = os.path.join(OBJ, out)
        if not os.path.exists(out) or open(out).read() != text:
            open(out, "w").write(text)


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


_digests = {}


def _code_digest(path):
    """digest of a header's CODE (comments and white space removed): an edit to a comment of include/ddp_amd.h does not recompile
    eighteen translation units (four minutes)"""
    if path not in _digests:
        txt = open(path).read()
        txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
        txt = re.sub(r"//[^\n]*", " ", txt)
        _digests[path] = hashlib.sha1(" ".join(txt.split()).encode()).hexdigest()
    return _digests[path]


def _save_usage(obj, stderr):
    """registers, scratch and LDS of every kernel of a translation unit, from the compiler's kernel-resource-usage remarks ->
    build/<unit>.usage.json (tests/test_capi_cpu.py: the kernels that count their own vector-memory operations — s_waitcnt vmcnt(N)
    with N from the number of loads they issue — must not spill to scratch: a spill is a vector-memory operation the count does not know)"""
    import json
    out, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass-analysis", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    json.dump(out, open(obj + ".usage.json", "w"), indent=0)


def _compile(src):
    obj = os.path.join(OBJ, src.replace(".hip", ".o"))
    hdrs = [os.path.join(CSRC, h) for h in HEADERS + EXTRA_DEPS.get(src, [])]
    stamp = obj + ".hdr"
    want = "\n".join("%s %s" % (os.path.basename(h), _code_digest(h)) for h in hdrs) + "\n" + " ".join(FLAGS + EXTRA_FLAGS.get(src, []))
    have = open(stamp).read() if os.path.exists(stamp) else None
    if _stale(obj, [os.path.join(CSRC, src)]) or have != want:
        cmd = ["hipcc"] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-c", os.path.join(CSRC, src), "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr[-4000:]))
        _save_usage(obj, r.stderr)
        open(stamp, "w").write(want)
        return src, True
    return src, False


def build(force=False, verbose=True):
    os.makedirs(OBJ, exist_ok=True)
    if force:
        for f in os.listdir(OBJ):
            os.remove(os.path.join(OBJ, f))
    _program_texts()
    srcs = [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    with cf.ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        results = list(ex.map(_compile, srcs))
    objs = [os.path.join(OBJ, s.replace(".hip", ".o")) for s in srcs]
    if any(changed for _, changed in results) or _stale(LIB, objs):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + ["-ldl"])
    if verbose:
        print("libddp_amd.so:", ", ".join("%s%s" % (s, "*" if c else "") for s, c in results))
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
