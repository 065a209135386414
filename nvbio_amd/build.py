"""Builds libnvbio_hip.so (the C-ABI library holding every gfx950 kernel) in-tree.

hipcc cross-compiles for gfx950 without a GPU; the .so is git-ignored but travels
to the GPU box with the repo snapshot.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libnvbio_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-fopenmp",
         "-Wno-unused-result", "-Wno-deprecated-declarations"]


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _deps(src):
    d = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    d.append(os.path.join(HERE, "..", "include", "nvbio_hip.h"))
    if os.path.basename(src) == "host_twins.hip":       # the only TU that instantiates the drop-in templates
        compat = os.path.join(HERE, "..", "include", "nvbio_hip", "compat")
        d += [os.path.join(r, f) for r, _, fs in os.walk(compat) for f in fs]
    return d


def _stale(target, srcs):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in srcs)


def _pool_size():
    """compilers to run at a time: MAX_JOBS when it is set to a positive number, else one per CPU"""
    try:
        jobs = int(os.environ.get("MAX_JOBS", "0"))
    except ValueError:
        jobs = 0
    return jobs if jobs > 0 else (os.cpu_count() or 1)


def build(force=False, verbose=False):
    os.makedirs(LIBDIR, exist_ok=True)
    objdir = os.path.join(LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    objs = []
    for src in sources():
        obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
        objs.append(obj)
        if force or _stale(obj, [src] + _deps(src)):
            jobs.append([HIPCC] + FLAGS + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)

    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), _pool_size())) as ex:
            list(ex.map(run, jobs))
    if jobs or force or _stale(LIB, objs):
        run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-fopenmp", "-o", LIB] + objs + ["-ldl"])
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
