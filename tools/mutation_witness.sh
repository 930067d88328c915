#!/bin/bash
# Mutation record of tests/test_witness_programs_gpu.py (profiles/mutation_witness.md).  Eleven scratch builds of the library, each with ONE
# defect in the GPU witness interpreter (witness.hip).  A mutant changes which value is computed or which in-range slot is read: the
# LDS ring index stays inside the ring, the table row inside the table, the flag index inside the flag array; none moves a global
# address, a loop bound or a synchronisation.  Nothing in the tree is modified: the copies are built under $W from a copy of the
# sources, the tree's other objects are linked in, and the tests load them through ZKHIP_LIB.
#   tools/mutation_witness.sh build [NAME] compile the mutants (CPU only; needs build/*.o from __graft_entry__.build())
#   tools/mutation_witness.sh run [NAME]   per mutant: the existing witness tests (test_witness_gpu.py, test_app_cache_gpu.py), then
#                                          the new file; each once, under its own time limit; prints one table row per mutant
# A run stops at the first exit status other than 0 (passed) or 1 (tests failed): the mutant is not run further, nor the next one.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=${ZKHIP_MUTANT_DIR:-$ROOT/build/mutants_witness}
MUTANTS="ring_lo_one_chunk_generous ring_lo_two_chunks_generous ring_read_half w_reduce_q_plus_1 subk_row_plus_1 subk_row_minus_1 chain_ring_ge chain_ring_two_generous inv_no_cond_sub flags_by_workgroup bit_rb_plus_1"

mutate() {      # name dir: exact replacements (each line must occur exactly once)
  python3 - "$1" "$2" <<'EOF'
import sys
name, d = sys.argv[1], sys.argv[2]
RING_LO = "const uint32_t w = (i + 1) * 64; return max(c0 * 64, w > WIT_RING ? w - WIT_RING : 0u);"
M = {
    # the ring is trusted for one chunk more than ring_lo allows: positions the reading chunk is about to overwrite
    "ring_lo_one_chunk_generous": [(RING_LO, "const uint32_t w = (i + 1) * 64; return max(c0 * 64, w > WIT_RING + 64 ? w - WIT_RING - 64 : 0u);")],
    # ... for two chunks more: positions the previous chunk overwrote
    "ring_lo_two_chunks_generous": [(RING_LO, "const uint32_t w = (i + 1) * 64; return max(c0 * 64, w > WIT_RING + 128 ? w - WIT_RING - 128 : 0u);")],
    # operands read from the ring at index mod RING / 2 (inside the ring, the wrong half for every second chunk pair)
    "ring_read_half": [("w_ld(&ring[((uint32_t)cur.a % WIT_RING) * 4])", "w_ld(&ring[((uint32_t)cur.a % (WIT_RING / 2)) * 4])"),
                       ("w_ld(&ring[((uint32_t)cur.b % WIT_RING) * 4])", "w_ld(&ring[((uint32_t)cur.b % (WIT_RING / 2)) * 4])")],
    # w_reduce subtracts one multiple of r too many
    "w_reduce_q_plus_1": [("const uint32_t q = (uint32_t)(((uint64_t)t * mu) >> 32);", "const uint32_t q = (uint32_t)(((uint64_t)t * mu) >> 32) + 1;")],
    # a - b + 2^k r adds the next row of the table (clamped to the table)
    "subk_row_plus_1": [("w_ld(&subk[(c - WT_SUBK) * 4])", "w_ld(&subk[min(c - WT_SUBK + 1, (uint32_t)WT_SUBK_LEVELS - 1) * 4])")],
    # ... the previous row (clamped): 2^(k-1) r is not enough for a subtrahend above it
    "subk_row_minus_1": [("w_ld(&subk[(c - WT_SUBK) * 4])", "w_ld(&subk[(max(c - WT_SUBK, 1u) - 1) * 4])")],
    # the chain's ring test one entry too generous (the entry the current instruction is about to overwrite), and two
    "chain_ring_ge": [("if ((uint32_t)ref + 64 > p) return", "if ((uint32_t)ref + 64 >= p) return")],
    "chain_ring_two_generous": [("if ((uint32_t)ref + 64 > p) return", "if ((uint32_t)ref + 65 >= p) return")],
    # the inversions take their operand as it comes (up to 4r) instead of below 2r
    "inv_no_cond_sub": [("r = fp_inv<FrParams>(fp_cond_sub_kp<FrParams, 2>(x));", "r = fp_inv<FrParams>(x);")],
    # k_witness raises the flag of the workgroup's number instead of the batch's (inside the flag array: there are fewer workgroups than batches)
    "flags_by_workgroup": [("if (bad) atomicOr(&flags[batch], 1u);", "if (bad) atomicOr(&flags[blockIdx.x], 1u);")],
    # WT_BIT reads the next bit (clamped to the 384 the words hold)
    "bit_rb_plus_1": [("r = ((w[rb >> 5] >> (rb & 31)) & 1u) ?", "const int32_t rb1 = min(rb + 1, 383);\n      r = ((w[rb1 >> 5] >> (rb1 & 31)) & 1u) ?")],
}
p = d + "/witness.hip"
s = open(p).read()
for old, new in M[name]:
    assert s.count(old) == 1, (name, old, s.count(old))
    s = s.replace(old, new)
open(p, "w").write(s)
print("mutated", name)
EOF
}

if [ "$1" = build ]; then
  [ -n "$2" ] && MUTANTS="$2"
  [ -f $ROOT/build/witness.o ]
  [ -n "$2" ] || rm -rf $W
  mkdir -p $W
  for m in $MUTANTS; do
    mkdir -p $W/$m/include $W/$m/zecale_amd                  # (witness.hip includes ../../include/zkhip.h)
    cp -r $ROOT/zecale_amd/csrc $W/$m/zecale_amd/csrc
    cp $ROOT/include/*.h* $W/$m/include/
    mutate $m $W/$m/zecale_amd/csrc
    ( hipcc --offload-arch=gfx950 -O3 -std=c++17 -DZK_MUL_INLINE=1 -fPIC -c $W/$m/zecale_amd/csrc/witness.hip -o $W/$m/witness.o &&
      objs="$W/$m/witness.o $(ls $ROOT/build/*.o | grep -v '/witness\.o$')" &&      # every object of the tree but the one rebuilt here
      hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o $W/$m/libzkhip.so $objs && rm -rf $W/$m/zecale_amd $W/$m/include $W/$m/witness.o && echo "built $m" ) &
  done
  wait
  for m in $MUTANTS; do [ -f $W/$m/libzkhip.so ] || { echo "missing $W/$m/libzkhip.so"; exit 1; }; done
  exit 0
fi

[ "$1" = run ] || { echo "usage: $0 build | run [NAME]"; exit 2; }
[ -n "$2" ] && MUTANTS="$2"
cd $ROOT
OLD="tests/test_witness_gpu.py tests/test_app_cache_gpu.py"
NEW="tests/test_witness_programs_gpu.py"
set +e
echo "| mutant | existing witness tests | new tests |"
echo "|---|---|---|"
for m in $MUTANTS; do
  lib=$W/$m/libzkhip.so
  [ -f $lib ] || { echo "missing $lib"; exit 1; }
  ZKHIP_LIB=$lib timeout -k 10 600 python -m pytest $OLD -x -q -p no:cacheprovider > $W/$m.old.txt 2>&1
  old=$?
  if [ $old -ne 0 ] && [ $old -ne 1 ]; then echo "| $m | exit $old: stopped |  |"; tail -20 $W/$m.old.txt; exit $old; fi
  ZKHIP_LIB=$lib timeout -k 10 300 python -m pytest $NEW -x -q -p no:cacheprovider > $W/$m.new.txt 2>&1
  new=$?
  if [ $new -ne 0 ] && [ $new -ne 1 ]; then echo "| $m | exit $old | exit $new: stopped |"; tail -20 $W/$m.new.txt; exit $new; fi
  verdict() { if [ $1 -eq 1 ]; then echo "killed: $(grep -m1 '^FAILED' $2 | cut -d' ' -f2 | cut -c1-120)"; else echo "survived ($(tail -1 $2 | tr -d '='))"; fi; }
  echo "| $m | $(verdict $old $W/$m.old.txt) | $(verdict $new $W/$m.new.txt) |"
done
