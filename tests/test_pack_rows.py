"""The row table of the packed-weight caches (medicalseg_amd/csrc/msk_pack_rows.h) is plain host C++: tests/pack_rows_main.cpp
drives every path of it at capacity 4 -- lookup, free-row and LRU claims, invalidation, drops, the in-use window, teardown --
as a stand-alone program built with AddressSanitizer and UBSan.  No GPU, nothing loaded into this process."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_pack_rows_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pack_rows_main")
    # (the sanitizer runtimes are linked statically: the program then does not care what else the loader brings in first)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "medicalseg_amd", "csrc"),
                           "-o", exe, os.path.join(HERE, "pack_rows_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all cases passed" in out.stdout
