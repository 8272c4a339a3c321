#!/bin/bash
# kernel_registers.sh [source.hip] — register / spill / LDS table of one source file's kernels (default poa_kernel.hip) from the
# compiler's resource-usage remarks (no GPU needed).
R=$(cd "$(dirname "$0")/.." && pwd)
SRC=${1:-poa_kernel.hip}
cd /tmp && hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -DHYPO_BUILD_ID=\"x\" -c $R/hypo_amd/csrc/$SRC \
    -Rpass-analysis=kernel-resource-usage -o /tmp/${SRC%.hip}_dev.o 2>&1 | python3 -c '
import re, sys
print("kernel,sgprs,sgpr_spills,vgprs,vgpr_spills,lds_bytes,waves_per_simd_by_vgprs,scratch_bytes_per_lane,occupancy_waves_per_simd")
cur = {}
def short_name(n):
    m = re.search(r"PoaCfgILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)", n)
    if m: return f"poa_class_kernel<GW={m.group(1)} CPL={m.group(2)} LMAX={m.group(3)} NMAX={m.group(4)}>"
    m = re.match(r"_ZN4hypo(\d+)", n)                  # hypo::<name>, then the integer template arguments if there are any
    if not m: return n[:40]
    name, tail = n[m.end():][:int(m.group(1))], n[m.end() + int(m.group(1)):]
    t = re.match(r"I((?:Li\d+E)+)E", tail)
    return name + ("<" + " ".join(re.findall(r"Li(\d+)E", t.group(1))) + ">" if t else "")
def flush():
    if cur.get("Name"):
        v = int(cur["VGPRs"])
        print(",".join([short_name(cur["Name"]), cur["TotalSGPRs"], cur["SGPRs Spill"], str(v), cur["VGPRs Spill"], cur["LDS Size [bytes/block]"],
                        str(512 // ((v + 7) // 8 * 8)), cur["ScratchSize [bytes/lane]"], cur["Occupancy [waves/SIMD]"]]))
for line in sys.stdin:
    m = re.search(r"remark:\s+(Function Name|[A-Za-z ]+(?: \[[^\]]+\])?): (\S+)", line)
    if not m: continue
    k, val = m.group(1).strip(), m.group(2)
    if k == "Function Name": flush(); cur.clear(); cur["Name"] = val
    else: cur[k] = val
flush()'
