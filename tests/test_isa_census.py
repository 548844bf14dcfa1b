"""The streaming kernel's register budget, checked on the code object inside the built library (no GPU): the production
instance -- K = 6, no lp, no multiplicities, float atomics -- must use no scratch memory and at most 128 vector registers,
i.e. run four waves per SIMD.  A spill's reload drains the LDS-DMA ring, and a compiler bump used to be the
only thing that told.  tools/probe/isa_census.py reads the kernel's metadata and disassembly; it also reports LDS-DMA
instructions that follow a VALU write of their SGPR base too closely (the hazard the inline assembly has to cover itself)."""
import json
import os
import subprocess
import sys

from conftest import ROOT

LIB = os.path.join(ROOT, "polee_amd", "csrc", "libpolee_hip.so")
CENSUS = os.path.join(ROOT, "tools", "probe", "isa_census.py")


def census(*args):
    r = subprocess.run([sys.executable, CENSUS, "--json", *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout)


def test_production_stream_kernel_keeps_its_register_budget():
    assert os.path.exists(LIB), "libpolee_hip.so is not built (make -C polee_amd/csrc)"
    kernels = census("--lib", LIB)["lib"]["kernels"]
    assert len(kernels) == 1, sorted(kernels)
    (name, k), = kernels.items()
    print(name, {key: k[key] for key in ("vgpr", "agpr", "sgpr", "scratch", "spilled_vgprs", "spilled_sgprs", "waves_per_simd")})
    assert k["scratch"] == 0 and k["spilled_vgprs"] == 0, k
    assert k["vgpr"] <= 128, k
    assert k["waves_per_simd"] == 4, k
    assert k["max_threads"] == 256, k
    assert k["mix"]["MFMA"] > 0 and k["mix"]["lds_dma"] > 0  # (the disassembly was read)
    assert k["dma_hazards"] == [], k["dma_hazards"]


def test_every_stream_kernel_instance_is_free_of_scratch_and_dma_hazards():
    kernels = census("--lib", LIB, "--kernel", "loglik_stream_kernel")["lib"]["kernels"]
    assert len(kernels) == 8 * 8, len(kernels)  # K = 1 .. 8 x (lp, multiplicities, deterministic)
    for name, k in kernels.items():
        assert k["scratch"] == 0 and k["spilled_vgprs"] == 0, (name, k["scratch"], k["spilled_vgprs"])
        assert k["waves_per_simd"] >= 3, (name, k["vgpr"])
        assert k["dma_hazards"] == [], (name, k["dma_hazards"])
