"""csrc/host_threads.h alone, as a stand-alone program (tests/host_threads_main.cpp includes nothing else of the project): for n in
{0, 1, 15, 16, 17, 1000} x grain in {1, 16, 64} x nt in {0, 1, 2, 16, n + 5} every index is visited exactly once, run_on_threads hands out
the worker numbers 0 .. max(1, nt) - 1 once each with worker 0 (and everything when nt <= 1) on the calling thread, and for_each_on_threads
never has more workers than ceil(n / grain).  Built plain, and a second time under ThreadSanitizer where the toolchain has its runtime."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_threads_main.cpp")
INC = os.path.join(ROOT, "mm2-gb_amd", "csrc")


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise RuntimeError("no host C++ compiler found")


def _build(exe, *flags):
    cmd = [_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", *flags, "-I", INC, SRC, "-o", str(exe)]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 90 cases"), r.stdout + r.stderr


def test_helper_alone(tmp_path):
    r = _build(tmp_path / "host_threads")
    assert r.returncode == 0, r.stderr
    _run(tmp_path / "host_threads")


def test_helper_alone_under_thread_sanitizer(tmp_path):
    r = _build(tmp_path / "host_threads_tsan", "-fsanitize=thread")
    if r.returncode != 0 and ("tsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this toolchain has no ThreadSanitizer runtime")
    assert r.returncode == 0, r.stderr
    _run(tmp_path / "host_threads_tsan")
