"""The fuse launch (k_update_insert) and the row move (k_move_rows, csrc/ssf_track_fuse.hip) run on the serial track chain beside the
extract waves.  A compute unit of the MI355X admits min(8, 800 // (ceil(sgpr / 16) * 16 + 16)) workgroups of 256 threads by scalar
registers: left alone both kernels take 104-106 (six per compute unit); amdgpu_num_sgpr caps the move at 80 (eight) and the fuse
launch at 96 (seven), which paid in the same-box A/B of profiles/move_icp_fused.txt.  The fused move keeps a row (29 words) in registers across its two ICP
gathers: it must stay at six waves per SIMD (80 vector registers) without scratch.  A compiler that no longer honours the caps, or
meets them by spilling, would silently take the gain back.  No GPU needed: the figures are the compiler's resource remarks."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "supersurfel_fusion_amd", "csrc")
FLAGS = ("--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt "
         "--offload-device-only -Rpass-analysis=kernel-resource-usage").split()
MOVE = "_ZN3ssf11k_move_rowsILb%dELb%dEE"
KERNELS = {"k_update_insert": "_ZN3ssf15k_update_insertE", "k_move_rows<false,false>": MOVE % (0, 0),
           "k_move_rows<true,false>": MOVE % (1, 0), "k_move_rows<true,true>": MOVE % (1, 1)}
CAP = {"k_update_insert": (96, 7), "k_move_rows<false,false>": (80, 8), "k_move_rows<true,false>": (80, 8), "k_move_rows<true,true>": (80, 8)}


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """name -> (scalar registers, vector registers, scratch bytes per lane) of the kernels above: one compilation, shared"""
    out = tmp_path_factory.mktemp("track_resources") / "tf.o"
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-c", "ssf_track_fuse.hip", "-o", str(out)], cwd=CSRC,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    res = {}
    for name, mangled in KERNELS.items():
        mine = [b for b in blocks if b.split("\n")[0].startswith(mangled)]
        assert len(mine) == 1, (name, [b.split("\n")[0] for b in mine])

        def g(key):
            return int(re.search(re.escape(key) + r": (\d+)", mine[0]).group(1))
        res[name] = (g("SGPRs"), g("VGPRs"), g("ScratchSize [bytes/lane]"))
        print("%s: %d sgpr, %d vgpr, %d B scratch" % ((name,) + res[name]))
    return res


def admitted_by_sgpr(sgpr):
    return min(8, 800 // (((sgpr + 15) // 16) * 16 + 16))


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_the_scalar_register_cap_holds_without_scratch(name, resources):
    sgpr, vgpr, scratch = resources[name]
    cap, admitted = CAP[name]
    assert sgpr <= cap and admitted_by_sgpr(sgpr) == admitted, (name, sgpr)
    assert scratch == 0, (name, scratch)


def test_the_fused_move_keeps_six_waves_per_simd(resources):
    for name in ("k_move_rows<true,false>", "k_move_rows<true,true>"):
        sgpr, vgpr, scratch = resources[name]
        assert vgpr <= 80 and 512 // (((vgpr + 7) // 8) * 8) >= 6, (name, vgpr)
    assert resources["k_update_insert"][1] <= 72 and resources["k_move_rows<false,false>"][1] <= 72     # seven, as before
