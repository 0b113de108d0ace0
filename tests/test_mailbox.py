"""The two self-validating record formats of the mailbox (csrc/ssf_mailbox.hpp: the ICP record's five lines and the integer
records of the counters and the shard sizes, their check words, and one attempt of the host's read -- what icp_fetch, fuse_end
and comm_counts call): tests/cpp/mailbox_smoke.cpp, a program of its own over the part that includes no HIP header, built with
the address and undefined-behaviour sanitizers and run as a process."""
import os
import subprocess

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")


def test_mailbox_records_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "mailbox_smoke")
    cmd = ["g++", "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CPP, "mailbox_smoke.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and "mailbox_smoke ok" in r.stdout, r.stdout
