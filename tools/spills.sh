#!/bin/bash
# register / scratch use of every kernel (CPU only: compiles each source to assembly and reads the code-object metadata).
# A latency-bound kernel that starts to spill gets slower without failing anything: run this after changing one.
cd "$(dirname "$0")/../zarc_amd/csrc" || exit 1
for f in *.hip; do
  fl=""; case $f in zge_entropy.hip|zstd_decode.hip) fl="-mllvm -amdgpu-sched-strategy=max-ilp";; zge_match.hip) fl="-mllvm -greedy-reverse-local-assignment=1 -mllvm -greedy-regclass-priority-trumps-globalness=1";; esac   # (the Makefile's FLAGS_*)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../../include -I. --cuda-device-only -S $fl -o /tmp/spills_$$.s $f 2>/dev/null || continue
  grep "\.name:\|\.private_segment_fixed_size\|\.vgpr_spill_count\|\.vgpr_count\|\.sgpr_spill_count\|\.group_segment_fixed_size" /tmp/spills_$$.s | paste - - - - - - |
    sed 's/  */ /g; s/\.group_segment_fixed_size/lds/; s/\.private_segment_fixed_size/scratch/; s/\.name: _Z[0-9]*\([a-z0-9_]*[a-z]\)[^ \t]*/\1/'
  # the match finder's memory waits: flat_ instructions per kernel (a window load through a pointer rebuilt from an integer is one: it
  # must be 0), and the vector-memory waits inside the level-3 kernel's tile loop (loop depth >= 3: units, blocks, tiles), full drains
  # (vmcnt(0)) against counted ones.  A kernel is taken to end at its first s_endpgm (today's finder kernels have one exit each): were
  # the compiler to emit an early exit, the waits behind it would be missing from the count.  Only the level-3 kernel is counted, so
  # the counters are never reset.  s_barrier: the workgroup barriers of that loop, rare paths included.
  if [ $f = zge_match.hip ]; then
    awk '/^_Z[0-9]+zarc_zge_match[a-z_]*9ZgeParams[A-Za-z0-9_]*:/ { k = $0; sub(/^_Z[0-9]+/, "", k); sub(/9ZgeParams.*/, "", k); d = 0 }
         /s_endpgm/ { if (k != "") { printf " %s flat_: %d", k, fl[k]; if (k == "zarc_zge_match") printf "  tile loop vmcnt(0): %d  vmcnt(N>0): %d  s_barrier: %d", z, c, sb; printf "\n" } k = "" }
         k != "" && (/^\.LBB/ || /^; %bb\./) { d = 0; if (match($0, /Depth=[0-9]+/)) d = substr($0, RSTART + 6, RLENGTH - 6) + 0 }
         k != "" && /^[ \t]+flat_/ { fl[k]++ }
         k == "zarc_zge_match" && d >= 3 && /s_waitcnt/ && /vmcnt\(0\)/ { z++ }
         k == "zarc_zge_match" && d >= 3 && /s_waitcnt/ && /vmcnt\([1-9]/ { c++ }
         k == "zarc_zge_match" && d >= 3 && /^[ \t]+s_barrier/ { sb++ }' /tmp/spills_$$.s
  fi
done
rm -f /tmp/spills_$$.s
