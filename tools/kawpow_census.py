#!/usr/bin/env python3
"""Static instruction census of the per-period KawPow search kernel.

Compiles one period of hip/kernels/kawpow_search.hip exactly as ops/jit.py does (the flags of
`_build.hipcc_genco`) with -save-temps, reads the gfx950 assembly the compiler leaves behind and
prints, for `kawpow_search`:

  * the resources from the code object's metadata: VGPRs, occupancy, LDS, private segment, spills;
  * VALU / LDS / vector-memory instruction counts per region of the kernel, where a region is a run
    of basic blocks (split at labels and branches): the seed keccak's block before the loop over
    the group's 16 hashes, that loop before / in / after the round loop, the final keccak's block
    after it, and whatever else is left (L1 fill, stale check, share store);
  * the wave64 VALU total per wave of 64 nonces: the hash loop runs 16 times and its round-loop
    block (16 unrolled rounds) 4 times per hash.

Instructions are classified by mnemonic prefix only (v_ = VALU, ds_ = LDS, buffer_ / global_ /
flat_ / scratch_ = vector memory); no particular instruction is looked for. No GPU is needed.

    python tools/kawpow_census.py --epoch 384                # the bench's period, tuned defines
    python tools/kawpow_census.py --epoch 390 --json         # the >= 4 GiB form (KP_PTR64)
    python tools/kawpow_census.py --period 960041 --defines KP_HASHES=1,KP_BLOCK=768
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNEL = "kawpow_search"
HASHES_PER_GROUP = 16   # trips of kp_group_hashes' outer loop at KP_HASHES=1
BLOCKS_PER_HASH = 4     # trips of the round loop: 64 rounds, 16 unrolled per trip
VMEM_PREFIXES = ("buffer_", "global_", "flat_", "scratch_")
REGIONS = ("seed keccak-f800 (kp_seed)", "per hash: mix init (KISS99)",
           "per hash: round-loop block (16 rounds)", "per hash: lane-hash reduce + digest placement",
           "final keccak-f800 (kp_final)", "elsewhere, not in the total (L1 fill, stale check, share store)")


def compile_asm(period: int, defines: tuple[str, ...], workdir: str) -> str:
    """Compile `period` with `defines` into `workdir`; returns the path of the device assembly."""
    from nodexa_chain_core_amd import _build
    from nodexa_chain_core_amd.ops import jit

    inc = os.path.join(workdir, f"kawpow_program_p{period}.inc")
    with open(inc, "w") as f:
        f.write(jit.program_source(period))
    _build.hipcc_genco(jit.TEMPLATE, os.path.join(workdir, "k.hsaco"),
                       defines=[f'KAWPOW_PROGRAM_HEADER="{inc}"', *defines], extra=["-save-temps=obj"])
    asm = [p for p in glob.glob(os.path.join(workdir, "*.s")) if "amdgcn" in os.path.basename(p)]
    if len(asm) != 1:
        raise RuntimeError(f"expected one device assembly file in {workdir}, found {asm}")
    return asm[0]


def _classify(mnemonic: str) -> str:
    if mnemonic.startswith("v_"):
        return "valu"
    if mnemonic.startswith("ds_"):
        return "lds"
    if mnemonic.startswith(VMEM_PREFIXES):
        return "vmem"
    return "other"


def basic_blocks(text: str, kernel: str = KERNEL) -> list[dict]:
    """The kernel's body as basic blocks: a new block starts at every label and after every branch.
    Each block: {"labels": [...], "valu", "lds", "vmem", "other", "target": label branched to or None}."""
    lines = text.splitlines()
    start = next(i for i, ln in enumerate(lines) if ln.startswith(kernel + ":"))
    blocks: list[dict] = []

    def new() -> dict:
        blocks.append({"labels": [], "valu": 0, "lds": 0, "vmem": 0, "other": 0, "target": None})
        return blocks[-1]

    cur = new()
    for ln in lines[start + 1:]:
        s = ln.split(";", 1)[0].strip()
        if not s:
            continue
        if s.startswith(".Lfunc_end"):
            break
        m = re.match(r"^([.\w$]+):$", s)
        if m:
            if cur["valu"] + cur["lds"] + cur["vmem"] + cur["other"] or cur["target"]:
                cur = new()
            cur["labels"].append(m.group(1))
            continue
        if s.startswith("."):
            continue  # directive
        mnemonic = s.split()[0]
        cur[_classify(mnemonic)] += 1
        if mnemonic.startswith(("s_cbranch", "s_branch")):
            cur["target"] = s.split()[-1]
            cur = new()
    return [b for b in blocks if b["labels"] or b["valu"] + b["lds"] + b["vmem"] + b["other"]]


def loops(blocks: list[dict]) -> list[tuple[int, int]]:
    """Back edges as (head, tail) block indices: a branch to a label at or before its own block."""
    where = {lab: i for i, b in enumerate(blocks) for lab in b["labels"]}
    return sorted((where[b["target"]], i) for i, b in enumerate(blocks)
                  if b["target"] in where and where[b["target"]] <= i)


def metadata(text: str, kernel: str = KERNEL) -> dict:
    """Resource figures of `kernel` from the code object's metadata (the .amdgpu_metadata notes the
    assembly carries) and the occupancy the compiler reports beside the kernel."""
    meta = text[text.index(".amdgpu_metadata"):]
    entries = re.split(r"\n\s+- \.agpr_count:", meta)
    entry = next(e for e in entries if re.search(r"\.name:\s+" + kernel + r"\s", e))

    def field(name: str) -> int:
        return int(re.search(r"\." + name + r":\s+(\d+)", entry).group(1))

    out = {"vgprs": field("vgpr_count"), "sgprs": field("sgpr_count"), "lds_bytes": field("group_segment_fixed_size"),
           "private_bytes": field("private_segment_fixed_size"), "vgpr_spills": field("vgpr_spill_count"),
           "sgpr_spills": field("sgpr_spill_count"), "max_threads": field("max_flat_workgroup_size")}
    body = text[text.index("\n" + kernel + ":"):]
    m = re.search(r";\s*Occupancy:\s*(\d+)", body)
    # 512 VGPRs per SIMD lane on gfx950, allocated in blocks of 8, at most 8 waves per SIMD
    out["occupancy"] = int(m.group(1)) if m else min(8, 512 // (-(-out["vgprs"] // 8) * 8))
    return out


def census_of_asm(text: str) -> dict:
    blocks = basic_blocks(text)
    back = loops(blocks)
    inner_candidates = [(h, t) for h, t in back if not any((h2, t2) != (h, t) and h <= h2 and t2 <= t for h2, t2 in back)]
    if not inner_candidates:
        raise RuntimeError("no loop found in " + KERNEL)
    total = lambda h, t, k="valu": sum(b[k] for b in blocks[h:t + 1])  # noqa: E731
    rh, rt = max(inner_candidates, key=lambda ht: total(*ht))  # the round loop: the heaviest innermost loop
    outer = [(h, t) for h, t in back if h <= rh and rt <= t and (h, t) != (rh, rt)]
    if not outer:
        raise RuntimeError("the round loop is not inside a hash loop")
    gh, gt = min(outer, key=lambda ht: ht[1] - ht[0])  # the tightest loop around it
    # straight-line code outside the hash loop: the seed keccak is the heaviest block before it and
    # the final keccak the heaviest after it; what is left there (L1 fill, stale check, share
    # store) runs once per workgroup or for a share only and is listed apart, outside the total
    seed = max(range(0, gh), key=lambda i: blocks[i]["valu"])
    final = max(range(gt + 1, len(blocks)), key=lambda i: blocks[i]["valu"])
    spans = ([seed], range(gh, rh), range(rh, rt + 1), range(rt + 1, gt + 1), [final],
             [i for i in range(len(blocks)) if not gh <= i <= gt and i not in (seed, final)])
    weights = (1, HASHES_PER_GROUP, HASHES_PER_GROUP * BLOCKS_PER_HASH, HASHES_PER_GROUP, 1, 0)
    regions = []
    for name, idx, w in zip(REGIONS, spans, weights):
        r = {"region": name, "blocks": len(idx), "runs_per_wave": w}
        for k in ("valu", "lds", "vmem", "other"):
            r[k] = sum(blocks[i][k] for i in idx)
        r["valu_per_wave"] = r["valu"] * w
        regions.append(r)
    per_wave = sum(r["valu_per_wave"] for r in regions)
    out = metadata(text)
    out.update({"regions": regions, "valu_per_wave": per_wave, "valu_per_nonce": round(per_wave / 64, 1),
                "round_block": {k: regions[2][k] for k in ("valu", "lds", "vmem", "other")},
                "valu_per_round": round(regions[2]["valu"] / 16, 1)})
    return out


def census(period: int, defines: tuple[str, ...]) -> dict:
    with tempfile.TemporaryDirectory(prefix="kawpow_census_") as tmp:
        with open(compile_asm(period, defines, tmp)) as f:
            text = f.read()
    out = census_of_asm(text)
    out.update({"period": period, "defines": list(defines)})
    return out


def render(c: dict) -> str:
    rows = [f"period {c['period']}  {' '.join(c['defines'])}",
            f"VGPRs {c['vgprs']}  occupancy {c['occupancy']}  LDS {c['lds_bytes']} B  private segment "
            f"{c['private_bytes']} B  VGPR spills {c['vgpr_spills']}  SGPR spills {c['sgpr_spills']}",
            "", "| region | VALU | LDS | vector memory | runs per wave | VALU per wave | share |", "|---|---|---|---|---|---|---|"]
    for r in c["regions"]:
        rows.append(f"| {r['region']} | {r['valu']} | {r['lds']} | {r['vmem']} | {r['runs_per_wave']} | "
                    f"{r['valu_per_wave']} | {100 * r['valu_per_wave'] / c['valu_per_wave']:.1f} % |")
    rows.append(f"| **total** | | | | | **{c['valu_per_wave']} = {c['valu_per_nonce']} per nonce** | |")
    rows.append(f"\n{c['valu_per_round']} VALU per round")
    return "\n".join(rows)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--epoch", type=int, default=384, help="census the bench's period of this epoch (height epoch*7500+123)")
    ap.add_argument("--period", type=int, default=None, help="a period of its own (the epoch still picks the DAG form)")
    ap.add_argument("--defines", default=None, help="comma-separated defines instead of the tuned ones")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()

    from nodexa_chain_core_amd import _build, _core
    from nodexa_chain_core_amd.ops import jit

    _build.build_core()
    period = a.period if a.period is not None else (a.epoch * _core.EPOCH_LENGTH + 123) // 3
    base = jit.TUNED_DEFINES if a.defines is None else tuple(d for d in a.defines.split(",") if d)
    defines = jit.defines_for(_core.full_dataset_num_items(a.epoch) * 128, base)
    c = census(period, defines)
    print(json.dumps(c) if a.json else render(c))
    return 0


if __name__ == "__main__":
    sys.exit(main())
