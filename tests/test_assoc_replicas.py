"""The waiting ICP launch k_icp<false, 0> (csrc/ssf_track_fuse.hip) does a frame's association on its way out, and since the
association bids into per-XCD replicas of the table it also picks its replica there.  A compute unit of the MI355X admits eight
256-thread workgroups up to 80 scalar registers and seven from 82 on; versions of this kernel above 80 ran the whole track chain
4-6 % slower (SSF_ICP_NUM_SGPR).  It must also stay without scratch.  No GPU needed: the figures are the compiler's resource
remarks, read the way tests/test_kernel_resources.py reads them."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "supersurfel_fusion_amd", "csrc")
FLAGS = ("--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt "
         "--offload-device-only -Rpass-analysis=kernel-resource-usage").split()


def test_the_waiting_icp_kernel_keeps_eight_workgroups_per_compute_unit(tmp_path):
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-c", "ssf_track_fuse.hip", "-o", str(tmp_path / "tf.o")], cwd=CSRC,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    # ssf::k_icp<false, 0>: _ZN3ssf5k_icpILb0ELi0EEE...
    blocks = [b for b in re.split(r"remark: Function Name: ", r.stderr)[1:] if b.split("\n")[0].startswith("_ZN3ssf5k_icpILb0ELi0EEE")]
    assert len(blocks) == 1, [b.split("\n")[0] for b in blocks]

    def g(key):
        return int(re.search(re.escape(key) + r": (\d+)", blocks[0]).group(1))
    sgpr, vgpr, scratch = g("SGPRs"), g("VGPRs"), g("ScratchSize [bytes/lane]")
    print("k_icp<false, 0>: %d sgpr, %d vgpr, %d B scratch" % (sgpr, vgpr, scratch))
    assert sgpr <= 80 and scratch == 0, (sgpr, scratch)
    assert min(8, 800 // (((sgpr + 15) // 16) * 16 + 16)) == 8
