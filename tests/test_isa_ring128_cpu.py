"""Code-generation guard for conv_gemm_ring128_kernel (CPU: hipcc cross-compiles gfx950, no GPU needed), by the
method of test_isa_cpu.py: its main loop keeps three K stages of LDS-DMA in flight with `s_waitcnt vmcnt(8)`, and a
full `vmcnt(0)` drain between the loop's header and its last MFMA (what hipcc's wait-count pass falls back to in
front of the fragment reads when it cannot tell the DMA'd LDS from what is read) would cost the prefetch with
bit-identical results."""
import os
import re
import shutil
import subprocess

import pytest

from test_isa_cpu import CSRC, HIPCC, _kernels, _mfma_loop


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("python3") is None, reason="no hipcc")
def test_ring128_main_loop_keeps_counted_waits(tmp_path):
    out = tmp_path / "conv_gemm.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17", "-munsafe-fp-atomics",
                    "-S", os.path.join(CSRC, "conv_gemm.hip"), "-o", str(out)], check=True, capture_output=True,
                   timeout=600)
    seen = 0
    for name, lines in _kernels(out.read_text()).items():
        if not re.search(r"conv_gemm_ring128_kernel", name):
            continue
        lo, hi = _mfma_loop(lines)
        assert hi > lo, name
        body = lines[lo:hi]
        assert re.search(r"s_cbranch\w*\s+\.LBB", lines[hi]), "%s: its MFMAs are in no loop" % name
        drains = sum("vmcnt(0)" in l for l in body)
        assert drains == 0, "%s: %d full vmcnt drains in its MFMA loop" % (name, drains)
        assert sum("vmcnt(8)" in l for l in body) >= 1, "%s: the counted wait is gone" % name
        # one K stage per MFMA block: 4 LDS-DMA loads for its 16 MFMAs
        nm, nd = sum("v_mfma" in l for l in body), sum(bool(re.search(r"buffer_load_dwordx4.*\blds\b", l)) for l in body)
        assert nm % 16 == 0 and nd * 4 == nm, (name, nm, nd)
        seen += 1
    assert seen == 4, seen          # K split 1 / 2, with and without the BN-backward sums
