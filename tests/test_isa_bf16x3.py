"""Guard on loop 1 of the bf16x3 product kernel (csrc/gemm_bf16x3.hip, k_gemm_bf16x3<1>: what cfg2's three products run), read from
the SHIPPED library minidiff_amd/libmdhip.so as tests/test_isa_guard.py reads the fp32 kernels (scripts/isa_check.py report_bf16x3;
no GPU needed). Loop 1's gain over loop 0 is compiler behaviour that nothing else pins: the staging addresses are formed before the
loop (no scalar multiply left in it), the DMAs stay in the scalar-base form, the fold stays four scalar adds behind an MFMA (the
compiler pairs free-standing adds into v_pk_add_f32, measured slower beside MFMAs), and the written-out order fits the 256
registers that two waves per SIMD leave, without scratch."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
OBJ = os.path.join(ROOT, "minidiff_amd", "libmdhip.so")


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(OBJ):
        pytest.skip("minidiff_amd/libmdhip.so not built (run __graft_entry__.build())")
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    import isa_check
    return isa_check.report_bf16x3(OBJ)


def _check(k):
    # 48 MFMAs per wave and k-tile (two k16 steps x six products x four sub-tiles); the loop holds two k-tiles
    assert k["mfma_loop"] == 96, k
    # nine 1-KiB pieces per wave and k-tile, every one in the scalar-base + 32-bit lane offset form
    assert k["dma_loop"] == 18 and k["dma_loop_saddr"] == 18 and k["dma_loop_vaddr64"] == 0 and k["lshl_add_u64_loop"] == 0, k
    # the piece bases are formed before the loop: no scalar multiply in it
    assert k["s_mul_loop"] == 0, k
    # the fold: 64 scalar adds per k-tile, none packed
    assert k["v_add_f32_loop"] == 128 and k["v_pk_add_f32_loop"] == 0, k
    # one barrier per k-tile, no drain between it and the first fragment read, no staging through registers, no scratch, and two
    # waves per SIMD
    assert k["barrier_loop"] == 2 and k["vmcnt0_between_barrier_and_first_read"] == 0, k
    assert k["ds_write"] == 0 and k["scratch"] == 0 and k["vgprs"] <= 256, k


def test_bf16x3_loop_1_kernel_shape(isa):
    _check(isa)


@pytest.mark.gpu
def test_bf16x3_loop_1_kernel_shape_of_the_library_on_the_gpu_box(isa):
    """The same facts in the driver's `-m gpu` run: what is checked there is the very file that run loads."""
    _check(isa)
