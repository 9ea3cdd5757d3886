"""The per-call scratch arena (muopdb_amd/csrc/mdb_arena.h) on its own: tests/scratch_arena_check.cpp drives it with malloc / free
as the injected allocator under AddressSanitizer + UBSan (a stand-alone program; nothing sanitised is loaded into Python)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_scratch_arena_properties(tmp_path):
    exe = str(tmp_path / "scratch_arena_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "scratch_arena_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
