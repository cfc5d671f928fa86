"""The exact float32 GEMM's fast-epilogue kernels -- the ones every Linear layer of the estimator launches -- fit the 128
registers of four waves per SIMD without spilling: no scratch, no VGPR or SGPR spill, as the compiler's resource report gives
them (hipcc -Rpass-analysis=kernel-resource-usage, the shipped -O3).  A spill there means scratch round trips in every tile
(DESIGN.md 3.1c).  CPU only: hipcc cross-compiles the unit for gfx950."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "notsofar1-challenge_amd", "csrc")
UNIT = os.path.join(CSRC, "gemm_f32.hip")
FIELDS = ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "VGPRs")


def _resource_usage():
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c",
                              "-Rpass-analysis=kernel-resource-usage", "-Wno-unused-value", "-I" + CSRC, UNIT,
                              "-o", os.path.join(d, "gemm_f32.o")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark: +([^:]+): (\d+)", line)
        if m and name and m.group(1).strip() in FIELDS:
            usage[name][m.group(1).strip()] = int(m.group(2))
    return usage


def test_fast_epilogue_kernels_do_not_spill():
    usage = _resource_usage()
    # gemm_f32_kernel<BD, FAST = true>: weights as fragments (the library's Linear layers) and from a row-major matrix
    fast = {k: v for k, v in usage.items() if re.search(r"gemm_f32_kernelILb[01]ELb1E", k)}
    assert len(fast) == 2, sorted(usage)
    for k, v in fast.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        assert v["VGPRs"] <= 128, (k, v)   # (__launch_bounds__(256, 4): four waves per SIMD)
