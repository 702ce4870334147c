"""Static census of the per-period KawPow search kernel (tools/kawpow_census.py): the bench's period
compiled with the tuned defines must keep its resource figures (80 VGPRs, 6 waves per SIMD, two
workgroups' LDS in a CU, nothing from memory in the round loop but the 16 DAG gathers) and must
not get the seed keccak it no longer recomputes back. No GPU: the compiler alone."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_PERIOD = (384 * 7500 + 123) // 3  # bench.py's height, epoch 384

# Wave64 VALU per wave of 64 nonces of the kernel before the seed was parked in LDS, counted the
# same way (seed block + 16 x (init + 4 x round-loop block + reduce) + final block): the
# structured-buffer form that runs at epoch 384, and the 64-bit-address form of the same period.
PARENT_VALU_PER_WAVE = {"KP_SBUFFER": 118_833, "KP_PTR64": 121_134}
# What parking the seed must save: one seed keccak-f800 (2,290 VALU in that census) less the slots'
# addressing (5 stores, 5 loads, the group's row: at most 76 VALU) and one instruction per
# round-loop block (64 runs per wave) of register-allocator noise.
CLAIMED_SAVING = 2_290 - 76 - 64


@pytest.fixture(scope="module")
def census_tool():
    spec = importlib.util.spec_from_file_location("kawpow_census", os.path.join(ROOT, "tools", "kawpow_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SYNTHETIC = """
\t.text
kawpow_search:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v1, 0
\ts_cbranch_execz .LBB0_9
\tv_add_u32_e32 v1, v1, v0
\tv_xor_b32_e32 v2, v1, v0
\tv_xor_b32_e32 v3, v2, v0
.LBB0_2:
\tds_read_b32 v4, v1
\tv_mul_lo_u32 v5, v4, v4
.LBB0_3:
\tbuffer_load_dwordx4 v[8:11], v5, s[0:3], 0 offen
\tds_read_b32 v6, v5
\tv_add_u32_e32 v5, v5, v6
\tv_xor_b32_e32 v5, v5, v8
\tv_xor_b32_e32 v5, v5, v9
\ts_cbranch_scc0 .LBB0_3
\tv_mov_b32_dpp v7, v5 row_newbcast:0
\ts_cbranch_scc1 .LBB0_2
\tv_xor_b32_e32 v1, v1, v7
\tv_xor_b32_e32 v1, v1, v7
\tv_xor_b32_e32 v1, v1, v7
\tv_xor_b32_e32 v1, v1, v7
\tglobal_store_dword v0, v1, s[0:1]
.LBB0_9:
\ts_endpgm
.Lfunc_end0:
"""


def test_census_regions_of_a_synthetic_kernel(census_tool):
    """Blocks split at labels and branches, the round loop is the heaviest innermost loop, the hash
    loop the tightest one around it; the total weighs them 64 and 16 times."""
    blocks = census_tool.basic_blocks(SYNTHETIC)
    assert [b["valu"] for b in blocks] == [1, 3, 1, 3, 1, 4, 0]
    assert census_tool.loops(blocks) == [(2, 4), (3, 3)]
    text = SYNTHETIC + """\t.amdgpu_metadata
amdhsa.kernels:
  - .agpr_count:     0
    .group_segment_fixed_size: 80900
    .max_flat_workgroup_size: 768
    .name:           kawpow_search
    .private_segment_fixed_size: 60
    .sgpr_count:     40
    .sgpr_spill_count: 0
    .vgpr_count:     80
    .vgpr_spill_count: 14
"""
    c = census_tool.census_of_asm(text)
    assert [r["valu"] for r in c["regions"]] == [3, 1, 3, 1, 4, 1]
    assert c["round_block"] == {"valu": 3, "lds": 1, "vmem": 1, "other": 1}
    assert c["valu_per_wave"] == 3 + 16 * (1 + 4 * 3 + 1) + 4
    assert (c["vgprs"], c["occupancy"], c["lds_bytes"], c["private_bytes"], c["vgpr_spills"]) == (80, 6, 80900, 60, 14)


@pytest.mark.parametrize("form", ["KP_SBUFFER", "KP_PTR64"])
def test_census_of_the_bench_period(core, census_tool, form):
    from nodexa_chain_core_amd.ops import jit

    if not jit.hipcc_available():
        pytest.skip("no hipcc on this machine")
    dag_bytes = (1 << 32) - 128 if form == "KP_SBUFFER" else 1 << 32
    defines = jit.defines_for(dag_bytes, jit.TUNED_DEFINES)
    assert form in defines
    c = census_tool.census(BENCH_PERIOD, defines)
    print(census_tool.render(c))
    assert c["vgprs"] == 80 and c["occupancy"] == 6
    assert c["lds_bytes"] <= 81_920  # two workgroups in a CU's 160 KiB
    assert c["round_block"]["vmem"] == 16  # the DAG gathers and nothing else from memory
    assert c["valu_per_wave"] <= PARENT_VALU_PER_WAVE[form] - CLAIMED_SAVING
