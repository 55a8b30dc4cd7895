"""The range and chunk arithmetic of the batch calls (csrc/query_plan.h: which records each device takes, the chunks of a range, the
event pairs that time them) without a GPU: tests/check_query_plan.cpp under AddressSanitizer + UBSan."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gpu_raytracer_amd", "csrc")


def test_ranges_and_chunks_cover_every_batch_exactly_once(tmp_path):
    """Every nd in 1 .. 8, chunk in {1, 1024, RT_QUERY_CHUNK / 4096, RT_QUERY_CHUNK, 2^24} and n in {0, 1, nd - 1, nd, chunk - 1, chunk,
    chunk + 1, 2 chunk + 5}, and n = 2^40 at chunk 2^24: 8 x (5 x 8 + 1) = 328 cases, as a host batch and as a device batch."""
    exe = str(tmp_path / "check_query_plan")
    run = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                          "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                          os.path.join(HERE, "check_query_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert re.search(r"^328 cases, 0 failures$", run.stdout.strip()), run.stdout[-500:]


def test_the_header_is_free_of_hip_and_only_the_runner_includes_it():
    text = open(os.path.join(CSRC, "query_plan.h")).read()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text) == ["cstddef"]
    users = [f for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f)) and '"query_plan.h"' in open(os.path.join(CSRC, f)).read()]
    assert users == ["rt_query.cpp"]
