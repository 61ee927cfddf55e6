"""Builds rslqr_amd/librslqr_amd.so in-tree: plain-C host library (gcc) + HIP shim/kernels
(hipcc --offload-arch=gfx950), linked into ONE shared object that exports the ndlqr_* C API of
include/ndlqr.h and the ndlqr_hip_* shim of include/ndlqr_hip.h.

    python -m rslqr_amd.build [--force]

hipcc cross-compiles gfx950 code objects without a GPU, so this runs anywhere ROCm is installed.
Every compile job writes its own dependency file (-MD -MF <obj>.d): an object is rebuilt when a file
it really includes, or this script, is newer than it.
"""
import concurrent.futures
import os
import re
import shlex
import shutil
import subprocess
import sys
import time

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(ROOT, "include")
OBJDIR = os.path.join(PKG, "build")
LIB = os.path.join(PKG, "librslqr_amd.so")
ARCH = "gfx950"

C_SOURCES = ["containers.c", "synth.c", "json.c", "batch.c", "solver.c", "linalg.c", "stages.c"]
HIP_MAIN = "ndlqr_hip.hip"            # the core: context, pipeline, the three families' launch sequences
# one unit per feature; a new feature adds its line here
HIP_UNITS = [HIP_MAIN, "hip_grad.hip", "hip_box.hip", "hip_refine.hip", "hip_cost.hip", "hip_lin.hip", "hip_lin_polish.hip", "hip_dense.hip",
             "hip_grad_dense.hip", "hip_gain.hip", "hip_objective.hip"]
HIP_INSTANCE = "small_instance.hip"   # compiled once per line of small_instances.def
HIP_REDUCED = "reduced_instance.hip"  # compiled once per tile count of the runtime-sized separator-only family
REDUCED_NB = range(1, 9)


def small_instances():
    """(nstates, ninputs) pairs listed in csrc/small_instances.def."""
    text = open(os.path.join(CSRC, "small_instances.def")).read()
    return [(int(a), int(b)) for a, b in re.findall(r"^NDLQR_SMALL_INSTANCE\((\d+),\s*(\d+)\)", text, flags=re.M)]


def hip_jobs():
    """(label, source file, extra flags, object file) of every HIP translation unit, in link order."""
    jobs = [("hipcc " + u, u, [], u + ".o") for u in HIP_UNITS]
    jobs += [("hipcc small instance (%d,%d)" % (nx, nu), HIP_INSTANCE, ["-DNDLQR_INST_NX=%d" % nx, "-DNDLQR_INST_NU=%d" % nu],
              "small_%d_%d.o" % (nx, nu)) for nx, nu in small_instances()]
    jobs += [("hipcc reduced instance NB=%d" % nb, HIP_REDUCED, ["-DNDLQR_RED_NB=%d" % nb], "reduced_%d.o" % nb)
             for nb in REDUCED_NB]
    return jobs


def hip_objects(skip=()):
    """Paths of the HIP objects the library links (those of the units in `skip` left out)."""
    return [os.path.join(OBJDIR, obj) for _, src, _, obj in hip_jobs() if src not in skip]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (set HIPCC)")


def hip_flags():
    return [_hipcc(), "--offload-arch=" + ARCH, "-std=c++17", "-O3", "-ffp-contract=off", "-fPIC", "-Wall",
            "-Wno-pass-failed",  # (13,4) with three fused levels misses its occupancy hint: expected
            "-I" + INCLUDE, "-I" + CSRC] + os.environ.get("NDLQR_EXTRA_HIPFLAGS", "").split()


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def _stale(obj):
    """An object is stale when it, or its dependency file, is missing or unreadable, or when a file that
    dependency file lists (or this script) is newer than it, or gone."""
    try:
        text = open(obj + ".d").read()
        deps = shlex.split(text.replace("\\\n", " ").split(":", 1)[1])
        t = os.path.getmtime(obj)
        return any(os.path.getmtime(d) > t for d in deps + [os.path.abspath(__file__)])
    except (OSError, IndexError, ValueError):
        return True


def _run(cmd):
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if proc.returncode != 0:
        sys.stderr.write(" ".join(cmd) + "\n" + proc.stdout + "\n")
        raise RuntimeError("build step failed: " + cmd[0])
    if proc.stdout.strip():
        sys.stderr.write(proc.stdout)


def _timed(cmd):
    t0 = time.time()
    _run(cmd)
    return time.time() - t0


def build(force=False, verbose=False):
    os.makedirs(OBJDIR, exist_ok=True)
    jobs, objs = [], []   # (label, command) for everything out of date
    for src in C_SOURCES:
        o = os.path.join(OBJDIR, src + ".o")
        if force or _stale(o):
            jobs.append(("cc " + src, ["gcc", "-std=gnu11", "-O2", "-g0", "-fPIC", "-Wall", "-Wextra", "-I" + INCLUDE,
                                       "-MD", "-MF", o + ".d", "-c", os.path.join(CSRC, src), "-o", o]))
        objs.append(o)
    flags = hip_flags()
    for label, src, extra, obj in hip_jobs():
        o = os.path.join(OBJDIR, obj)
        if force or _stale(o):
            jobs.append((label, flags + extra + ["-MD", "-MF", o + ".d", "-c", os.path.join(CSRC, src), "-o", o]))
        objs.append(o)
    if jobs:
        # the translation units are independent: compile them side by side (MAX_JOBS, where set, says how many
        # processors this build may use; a shared host reports more than that)
        cpus = int(os.environ["MAX_JOBS"]) if os.environ.get("MAX_JOBS", "").isdigit() else min(os.cpu_count() or 2, 16)
        workers = max(1, min(len(jobs), cpus))
        with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
            futures = {pool.submit(_timed, cmd): label for label, cmd in jobs}
            for fut in concurrent.futures.as_completed(futures):
                seconds = fut.result()
                if verbose:
                    print("%-40s %6.1f s" % (futures[fut], seconds))
    if force or _newer(LIB, objs):
        if verbose:
            print("link", os.path.basename(LIB))
        _run([flags[0], "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs + ["-lm", "-lpthread"])
    return LIB


if __name__ == "__main__":
    if "--hip-objects" in sys.argv:  # (oracle/Makefile: the sanitizer build links them as built)
        print(" ".join(hip_objects()))
    else:
        t_start = time.time()
        print(build(force="--force" in sys.argv, verbose=True))
        print("wall %.1f s" % (time.time() - t_start))
