#!/bin/bash
# the round's micro-benchmarks on the GPU box: gpurun_out/ubench/{imad,dfma}.txt (copy to profiles/rNN_*_ubench.txt)
# (and mont_carry.txt beside them, kept as profiles/r07_mont_carry_ubench.txt)
O=gpurun_out/ubench; mkdir -p $O
hipcc --offload-arch=gfx950 -O3 tools/ubench/imad.hip -o /tmp/imad > /dev/null 2>&1 && timeout -k 10 400 /tmp/imad > $O/imad.txt 2>&1; echo "imad rc=$?"
hipcc --offload-arch=gfx950 -O3 tools/ubench/dfma_mont.hip -o /tmp/dfma > /dev/null 2>&1 && timeout -k 10 300 /tmp/dfma > $O/dfma.txt 2>&1; echo "dfma rc=$?"
# mont_carry: the instruction counts of each form's kernel (one product in a loop plus ~110 instructions of loads, stores and loop
# control) from the compiled code, then the run
count_forms() {   # $1: the device assembly
  awk '/^_Z7k_chain[A-Za-z0-9_]*Li512E[A-Za-z0-9_]*:/ { name = $1 }
       name != "" && /^[ \t]+v_mad_u64_u32/ { mad++ } name != "" && /^[ \t]+v_lshl_add_u64/ { a64++ } name != "" && /^[ \t]+s_nop/ { nop++ }
       name != "" && /^[ \t]+v_/ { valu++ } name != "" && /^[ \t]+s_/ { salu++ }
       name != "" && /s_endpgm/ { split(name, f, /ILi|ELb|ELi/); split("a-plain b-asm-mad c-barrier d-asm-run e-copy", nm, " "); printf "# compiled: %s %-10s  v_mad_u64_u32 %d  other VALU %d  (v_lshl_add_u64 %d)  s_nop %d  other SALU %d\n", (f[3] == "1" ? "sqr" : "mul"), nm[f[2] + 1], mad, valu - mad, a64, nop, salu - nop; name = ""; mad = a64 = nop = valu = salu = 0 }' $1
}
( cd /tmp && hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S $OLDPWD/tools/ubench/mont_carry.hip -o /tmp/mont_carry.s > /dev/null 2>&1 ) && count_forms /tmp/mont_carry.s > $O/mont_carry.txt
hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench/mont_carry.hip -o /tmp/mont_carry > /dev/null 2>&1 && timeout -k 10 240 /tmp/mont_carry >> $O/mont_carry.txt 2>&1; echo "mont_carry rc=$?"
cat $O/dfma.txt
grep -E "^---|mad_u64_u32|mad64|add_u32" $O/imad.txt | cut -c1-330
cat $O/mont_carry.txt
