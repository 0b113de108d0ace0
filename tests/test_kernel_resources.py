"""The resident ICP launch (k_icp_resident, csrc/ssf_track_fuse.hip) waits on its own workgroups: all of them -- up to 1024 -- must
hold a place on the GPU at once.  How many places there are follows from the kernel's registers: a compute unit of the MI355X
admits min(8, 800 // (ceil(sgpr / 16) * 16 + 16)) workgroups of 256 threads by scalar registers and 512 // (ceil(vgpr / 8) * 8) by
vector registers (a workgroup is one wave on each of the four SIMDs).  The kernel is held at 72 vector registers by __launch_bounds__(256, 7) and a few register
barriers; a compiler that no longer honours them would silently shrink the margin the limit relies on.  No GPU needed: the
figures come from the compiler's resource remarks (what tools/kernel_resources.py prints)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "supersurfel_fusion_amd", "csrc")
FLAGS = ("--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt "
         "--offload-device-only -Rpass-analysis=kernel-resource-usage").split()
CUS, MAX_WGS = 256, 1024


def test_the_resident_icp_kernel_leaves_room_for_its_whole_grid(tmp_path):
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-c", "ssf_track_fuse.hip", "-o", str(tmp_path / "tf.o")], cwd=CSRC,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: Function Name: ", r.stderr)[1:] if "k_icp_resident" in b.split("\n")[0]]
    assert len(blocks) == 1, [b.split("\n")[0] for b in blocks]

    def g(key):
        return int(re.search(re.escape(key) + r": (\d+)", blocks[0]).group(1))
    sgpr, vgpr, scratch, lds = g("SGPRs"), g("VGPRs"), g("ScratchSize [bytes/lane]"), g("LDS Size [bytes/block]")
    by_sgpr = min(8, 800 // (((sgpr + 15) // 16) * 16 + 16))
    by_vgpr = (512 // (((vgpr + 7) // 8) * 8)) * 4 // 4          # waves per SIMD = 256-thread workgroups per compute unit
    by_lds = (160 * 1024) // max(lds, 1)
    places = CUS * min(by_sgpr, by_vgpr, by_lds, 8)
    print("k_icp_resident: %d sgpr, %d vgpr, %d B scratch, %d B LDS -> %d places" % (sgpr, vgpr, scratch, lds, places))
    assert sgpr <= 80 and vgpr <= 72 and scratch <= 16, (sgpr, vgpr, scratch)
    assert places >= 1792 and places >= MAX_WGS + 512, places
    src = open(os.path.join(CSRC, "ssf_track_fuse.hip")).read()
    assert "int icp_resident_max_wgs() { return %d; }" % MAX_WGS in src
