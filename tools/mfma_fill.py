#!/usr/bin/env python3
"""Diagnostic: what one more instruction of a given kind costs next to the fp32 MFMA stream (diagnostic library).
Per kind: added shader cycles per filler instruction and SIMD, at 1 to 3 waves per SIMD.
  --winograd   only the adds of the Winograd kernels at their own densities: scalar and packed (plain, negated, half-selecting)
               per 8 v_mfma_f32_32x32x2_f32 at one wave per SIMD (weight gradient: 22 scalar / 11 packed) and per 8
               v_mfma_f32_16x16x4_f32 at two (conv: 10 scalar / 5 packed)
  --rowsplit   what the one-row-per-wave weight gradient rests on, per 8 v_mfma_f32_32x32x2_f32 at one wave per SIMD:
               v_pk_fma_f32 and v_pk_add_f32 at 6, ds_read2st64_b32 at 6 against 5"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import sisr_amd  # noqa: E402

hip = sisr_amd.hip
L = hip.lib()
dev = torch.device("cuda:0")
KINDS = {1: "v_add_f32", 2: "v_and_b32", 3: "s_add_u32", 4: "ds_read_b128", 5: "global_load_dwordx4 (vaddr)", 6: "ds_write_b128",
         7: "global_store_dword", 8: "v_mov_b32", 9: "s_nop", 10: "v_pk_add_f32", 11: "v_lshl_add_u64",
         12: "global_load_dwordx4 (saddr)", 13: "v_pk_add_f32 neg_lo neg_hi", 14: "v_pk_add_f32 op_sel neg_lo neg_hi"}
ROWSPLIT = {15: "v_pk_fma_f32", 16: "ds_read2st64_b32"}  # priced by --rowsplit only
MFMAS = {0: "v_mfma_f32_32x32x2_f32", 1: "v_mfma_f32_16x16x4_f32"}
src = torch.zeros(1 << 16, device=dev)
iters = 4000


def run(wps, kind, count):
    blocks = 256 * wps
    out = torch.empty(blocks * 256, device=dev)
    clk = torch.zeros(2, dtype=torch.int64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(3):
        if rep == 2:
            e0.record()
        hip.check(L.sisr_diag_mfma_fill(blocks, iters, kind, count, hip.ptr(out), hip.ptr(src), clk.data_ptr(), hip.stream()), "fill")
    e1.record()
    torch.cuda.synchronize()
    c = clk.cpu().tolist()
    ghz = c[0] / max(c[1], 1) * 0.1
    # whole-launch time -> shader cycles one SIMD spends per loop iteration of ALL its waves
    return e0.elapsed_time(e1) * 1e6 * ghz / iters, ghz


if "--winograd" in sys.argv[1:]:
    for mf, wps, scalar, packed in ((0, 1, 22, 11), (0, 2, 22, 11), (1, 1, 10, 5), (1, 2, 10, 5), (1, 2, 16, 8)):
        base, ghz = run(wps, 1 + 100 * mf, 0)
        print(json.dumps({"mfma": MFMAS[mf], "waves_per_simd": wps, "kind": "none", "simd_cycles_per_iter": base, "GHz": ghz}), flush=True)
        for kind, count in ((1, scalar), (10, packed), (13, packed), (14, packed), (10, scalar)):
            cyc, _ = run(wps, kind + 100 * mf, count)
            print(json.dumps({"mfma": MFMAS[mf], "waves_per_simd": wps, "kind": KINDS[kind], "per_8_mfma": count,
                              "simd_cycles_per_iter": round(cyc, 1), "added_simd_cycles_per_filler": round((cyc - base) / (wps * count), 2)}),
                  flush=True)
    sys.exit(0)

if "--rowsplit" in sys.argv[1:]:
    base, ghz = run(1, 1, 0)
    print(json.dumps({"mfma": MFMAS[0], "waves_per_simd": 1, "kind": "none", "simd_cycles_per_iter": base, "GHz": ghz}), flush=True)
    for kind, count in ((15, 6), (10, 6), (15, 5), (16, 6), (16, 5)):
        cyc, _ = run(1, kind, count)
        print(json.dumps({"mfma": MFMAS[0], "waves_per_simd": 1, "kind": {**KINDS, **ROWSPLIT}[kind], "per_8_mfma": count,
                          "simd_cycles_per_iter": round(cyc, 1), "added_simd_cycles_per_filler": round((cyc - base) / count, 2)}),
              flush=True)
    sys.exit(0)

for wps in (1, 2, 3):
    base, ghz = run(wps, 1, 0)
    print(json.dumps({"waves_per_simd": wps, "kind": "none", "simd_cycles_per_iter": base, "GHz": ghz,
                      "ideal": 512 * wps}), flush=True)
    for kind, name in KINDS.items():
        row = {"waves_per_simd": wps, "kind": name}
        for count in (8, 16, 32):
            cyc, _ = run(wps, kind, count)
            row[f"added_simd_cycles_per_filler@{count}"] = round((cyc - base) / (wps * count), 2)
        print(json.dumps(row), flush=True)
