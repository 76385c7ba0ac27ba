"""Host-side ThreadSanitizer run of keto_snapshot_delete_query's locking
(tests/tsan_delete/delete_query_tsan.cpp): planners calling keto_list_plan while a writer alternates
keto_snapshot_delete_query and keto_snapshot_apply on one host-only snapshot.  The library's host code
is built with -fsanitize=thread as tests/test_tsan_host.py builds it (-Xarch_host for the .hip sources,
whose kernels never run here).  The driver has to finish -- the delete takes the list index's mutex
under the snapshot's shared lock, as list calls do, and never waits for the exclusive lock while it
holds the mutex -- and any data race fails the test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_delete_query_under_tsan(tmp_path):
    from concurrent.futures import ThreadPoolExecutor
    from keto_amd.build import HOST_HIP, SOURCES
    csrc = os.path.join(ROOT, "keto_amd", "csrc")
    san = ["-fsanitize=thread", "-fno-omit-frame-pointer"]

    def compile_one(f):
        o = str(tmp_path / (f + ".o"))
        if f.endswith(".cpp"):
            cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", *HOST_HIP, *san, "-c", os.path.join(csrc, f), "-o", o]
        else:
            cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                   "-fsanitize=thread", "-fno-omit-frame-pointer", "-w", "-c", os.path.join(csrc, f), "-o", o]
        subprocess.check_call(cmd)
        return o

    with ThreadPoolExecutor(4) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    d = str(tmp_path / "drv.o")
    subprocess.check_call([HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", *san, "-c",
                           os.path.join(ROOT, "tests", "tsan_delete", "delete_query_tsan.cpp"), "-o", d])
    exe = str(tmp_path / "delete_query_tsan")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-fsanitize=thread", "-fno-gpu-sanitize", d, *objs, "-o", exe,
                           "-L/opt/rocm/lib", "-lrccl"])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1:second_deadlock_stack=1", KETO_BUILD_THREADS="4")
    r = subprocess.run([exe, "200"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "tsan delete rounds ok: 200 deletes" in r.stdout
