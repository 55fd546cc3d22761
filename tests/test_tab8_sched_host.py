"""tools/ubench/tab8_sched.h on the host: the block schedules (static, claimed, hybrid) that the micro-benchmark
tools/ubench/stream4.hip times for the 64 KiB-table kernel.  Benchmark-only code: the library's kernels do not use the header, so
this checks the benchmark's variants, not the library.  tests/csrc/tab8_sched_host_test.cpp replays the schedules with the
workgroups advanced in a shuffled order and asserts that every vector in [0, n / 16) is covered exactly once and nothing beyond
it, for n in {0, 1, 15, 16, 17, one block +- 1, grid x block +- 16, 3 x grid x block + 5, 1e8}, five grids, two block sizes and every
static / claimed split."""
import os
import subprocess

import pytest


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_tab8_schedule_covers_every_vector_once_on_the_host(tmp_path, repo_root, sanitize):
    exe = str(tmp_path / "tab8_sched_test")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17"] + flags + ["-I", os.path.join(repo_root, "tools", "ubench"),
                    os.path.join(repo_root, "tests", "csrc", "tab8_sched_host_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "tab8 schedule ok" in r.stdout, r.stdout + r.stderr
