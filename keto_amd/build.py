"""Build recipe for the in-tree HIP library keto_amd/libketo_mi355x.so (gfx950 only)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libketo_mi355x.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
SOURCES = ["snapshot.cpp", "resolve.cpp", "delta.cpp", "persist.cpp", "capi.cpp", "engine.hip", "route.hip", "migrate.hip", "proto.hip", "reach.hip", "resolve_dev.hip", "list.hip", "subjects.hip", "allowed.hip", "comm.cpp"]
CXXFLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]
HOST_HIP = ["-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]   # host-only sources using the HIP / RCCL APIs
# engine.hip (tier 0, the deep tier, expand) and migrate.hip (the migrating walk) are scheduled for
# memory clauses: the latency-bound walks' independent loads issue back to back (config #3 126-128 ->
# 121 ms, P = 8 migrating parts 18.1-19.2 -> 17.3-18.1 ms; tier 0 and config #5 unchanged; A/B on one
# box: profiles/r06zzc_configs_compiler_flags.txt, r06zze_migrate_compiler_flags.txt, r06zzb_*)
_MEM_CLAUSE = ["-mllvm", "-amdgpu-sched-strategy=max-memory-clause"]
SOURCE_FLAGS = {"engine.hip": _MEM_CLAUSE, "migrate.hip": _MEM_CLAUSE}


def _csrc_includes(name, seen):
    """`name` and the csrc headers it includes, transitively, each once, in include order."""
    if name not in seen:
        seen.append(name)
        for line in open(os.path.join(CSRC, name), encoding="utf-8"):
            inc = line.split('"')[1] if line.startswith('#include "') else ""
            if inc and "/" not in inc and os.path.exists(os.path.join(CSRC, inc)):
                _csrc_includes(inc, seen)
    return seen


def engine_build_id():
    """sha256 of what the tier-0 check kernel is compiled from: engine.hip, the csrc headers it
    includes (hip_check.hpp, snapshot.hpp) and its compile flags.  Keys the committed PMC traffic
    profiles (tools/traffic.py writes it, bench.py matches it)."""
    import hashlib
    h = hashlib.sha256()
    for name in _csrc_includes("engine.hip", []):
        h.update(name.encode() + b"\0" + open(os.path.join(CSRC, name), "rb").read() + b"\0")
    h.update(" ".join(SOURCE_FLAGS.get("engine.hip", [])).encode())
    return h.hexdigest()


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile_cmd(src, obj, extra=()):
    path = os.path.join(CSRC, src)
    if src.endswith(".cpp"):
        return [HIPCC, *CXXFLAGS, *HOST_HIP, *extra, "-x", "c++", "-c", path, "-o", obj]
    return [HIPCC, f"--offload-arch={ARCH}", *CXXFLAGS, *SOURCE_FLAGS.get(src, []), *extra, "-c", path, "-o", obj]


def _link_cmd(objs, out):
    return [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", out, *objs, "-L/opt/rocm/lib", "-lrccl"]


def build(verbose=False, force=False):
    headers = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp"))
    headers += [os.path.join(HERE, "..", "include", "keto_mi355x.h"), os.path.abspath(__file__)]
    if not force and not _stale(OUT, [os.path.join(CSRC, s) for s in SOURCES] + headers):
        return OUT
    objs = []
    for src in SOURCES:
        obj = os.path.join(CSRC, src + ".o")
        objs.append(obj)
        if not force and not _stale(obj, [os.path.join(CSRC, src)] + headers):
            continue
        cmd = _compile_cmd(src, obj)
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    cmd = _link_cmd(objs, OUT)
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    build(verbose=True, force="--force" in sys.argv)


def build_variant(name, defines):
    """Tuning build with -D defines into keto_amd/variants/lib_<name>.so (select with KETO_LIB)."""
    vdir = os.path.join(HERE, "variants")
    os.makedirs(vdir, exist_ok=True)
    objs = []
    for src in SOURCES:
        obj = os.path.join(vdir, f"{name}_{src}.o")
        subprocess.check_call(_compile_cmd(src, obj, [f"-D{d}" for d in defines]))
        objs.append(obj)
    out = os.path.join(vdir, f"lib_{name}.so")
    subprocess.check_call(_link_cmd(objs, out))
    return out
