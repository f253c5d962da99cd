#!/bin/bash
# Static statistics of the main kernels for a set of extra compile flags:
#   tools/kstat.sh "<flags>"
# VGPR / scratch / occupancy from the compiler remarks, and instruction counts
# (VALU, SALU, scalar loads, scratch ops, vmcnt(0) waits, SGPR-spill lane ops)
# from the assembly.  The assembly stays in /tmp/kstat.s.
cd "$(dirname "$0")/../dwarf-p-cloudsc_amd" || exit 1
hipcc -O3 -ffp-contract=off -fPIC -std=c++17 --offload-arch=gfx950 -mllvm -disable-machine-licm -I../include -Icsrc \
  --cuda-device-only -S csrc/cloudsc_gpu.hip -o /tmp/kstat.s $1 -Rpass-analysis=kernel-resource-usage 2> /tmp/kstat.err || exit 1
# the product's plain unpacked kernels, by demangled name (kcache_entry<F> / kseg_entry<F>, F the form
# descriptor cloudsc::KForm<compute, storage, WAVES, PF, AER, LDSC, FAST, form bits>)
declare -A NAMES=(
  ["void kseg_entry<cloudsc::KForm<double, double, 2, 3, false, false, false, 0u>>"]="kseg<double,2,3>"
  ["void kcache_entry<cloudsc::KForm<double, double, 2, 3, false, false, false, 0u>>"]="kcache<double,2,3>"
  ["void kseg_entry<cloudsc::KForm<float, float, 2, 1, false, false, true, 0u>>"]="kseg<float,2,1,fast>"
  ["void kcache_entry<cloudsc::KForm<float, float, 2, 1, false, false, true, 0u>>"]="kcache<float,2,1,fast>"
)
for k in $(grep -E '^\s*\.amdhsa_kernel ' /tmp/kstat.s | awk '{print $2}'); do
  label=${NAMES[$(echo "$k" | c++filt | sed 's/>(.*$/>/')]}
  [ -n "$label" ] || continue
  awk "/^$k:/,/s_endpgm/" /tmp/kstat.s > /tmp/kstat_k.s
  res=$(grep -A12 "Function Name: $k" /tmp/kstat.err | grep -E "VGPRs:|ScratchSize|Occupancy" | head -3 |
        sed 's/.*remark: //;s/ \[-Rpass.*//;s/ \[bytes\/lane\]//;s/ \[waves\/SIMD\]//' | tr -s ' ' | tr '\n' ' ')
  printf "%-24s %s valu=%d salu=%d sload=%d lgkm=%d scratch=%d vmcnt0=%d lane=%d\n" "$label" "$res" \
    "$(grep -cE '^\s+v_' /tmp/kstat_k.s)" "$(grep -cE '^\s+s_' /tmp/kstat_k.s)" "$(grep -c 's_load' /tmp/kstat_k.s)" \
    "$(grep -c 'lgkmcnt' /tmp/kstat_k.s)" "$(grep -c 'scratch_' /tmp/kstat_k.s)" "$(grep -c 'vmcnt(0)' /tmp/kstat_k.s)" \
    "$(grep -c 'lane_b32' /tmp/kstat_k.s)"
done
