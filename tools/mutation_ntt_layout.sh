#!/bin/bash
# Mutation record of tests/test_ntt_layout_gpu.py (profiles/mutation_ntt_layout.md).  Four scratch builds of the library, each with ONE
# line of zecale_amd/csrc/ntt.hip changed.  A mutant changes arithmetic, a table's contents or which IN-RANGE element is touched - never
# a bound, a trip count, a synchronisation or an address outside a buffer or the LDS tile.  Nothing in the tree is modified: the copies are
# built under $W from a copy of the sources, the tree's other objects are linked in at their usual places, and the tests load them through
# ZKHIP_LIB.
#   tools/mutation_ntt_layout.sh build        compile the mutants (CPU only; needs build/*.o from __graft_entry__.build())
#   tools/mutation_ntt_layout.sh run [NAME]   per mutant: tests/test_ntt_gpu.py, then the new file; each under its own time limit; one
#                                             table row per mutant
# `build` STOPS with a message when a pattern it patches no longer occurs exactly once in ntt.hip: the script must follow the source.
# A run stops at the first exit status other than 0 (passed) or 1 (tests failed): the mutant is not run further, nor the next one.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=${ZKHIP_MUTANT_DIR:-$ROOT/build/mutants_ntt}
MUTANTS="post_k_transposed_side stage1_sub_2r batch_vector_0 wide_tile_load_swapped"

mutate() {      # name file: one exact replacement
  python3 - "$1" "$2" <<'EOF'
import sys
name, path = sys.argv[1], sys.argv[2]
M = {
    # (a) the inverse coset transform of TRANSPOSED input multiplies its second pass by the table of the natural side, (g^-K)^k where
    #     (g^-N2)^k belongs.  Patched where the table is made, with K entries kept: taking the pointer post_k[0] instead would read a table
    #     of N2 entries with k < K = 2 N2 at every odd size - outside the allocation.  K = N2 at even sizes: no difference there.
    "post_k_transposed_side": (
        "make_powers(hfr_pow_u64(h, N2), HFr::one(), K, &t.post_k[1])",
        "make_powers(hfr_pow_u64(h, K), HFr::one(), K, &t.post_k[1])"),
    # (b) the first stage subtracts as if its operands were below 2 r (the contract: below 8 r)
    "stage1_sub_2r": (
        "y0 = fp_add(x0, x1); y1 = fp_sub<FrParams, 16>(x0, x1);",
        "y0 = fp_add(x0, x1); y1 = fp_sub<FrParams, 2>(x0, x1);"),
    # (c) every vector of a batch is vector 0
    "batch_vector_0": (
        "uint32_t* const data = a.data[blockIdx.y];",
        "uint32_t* const data = a.data[0];"),
    # (d) load phase only: neighbouring sub-transforms of a wide tile change places in LDS (the identity for C = 1; inside the tile for any C)
    "wide_tile_load_swapped": (
        "const uint32_t pw = lds_sw(cc * K + rj);",
        "const uint32_t pw = lds_sw(((cc ^ 1u) & (C - 1)) * K + rj);"),
}
old, new = M[name]
s = open(path).read()
if s.count(old) != 1:
    sys.exit("mutation_ntt_layout.sh: the line of mutant '%s' occurs %d times in ntt.hip, not once:\n    %s\nupdate the pattern to the source before trusting the record" % (name, s.count(old), old))
open(path, "w").write(s.replace(old, new))
print("mutated", name)
EOF
}

if [ "$1" = build ]; then
  [ -f $ROOT/build/ntt.o ] || { echo "mutation_ntt_layout.sh: build the tree first (build/ntt.o is missing)"; exit 1; }
  rm -rf $W && mkdir -p $W
  for m in $MUTANTS; do
    mkdir -p $W/$m/include $W/$m/zecale_amd                  # (ntt.h includes ../../include/zkhip.h)
    cp -r $ROOT/zecale_amd/csrc $W/$m/zecale_amd/csrc
    cp $ROOT/include/*.h* $W/$m/include/
    mutate $m $W/$m/zecale_amd/csrc/ntt.hip
  done
  for m in $MUTANTS; do
    ( hipcc --offload-arch=gfx950 -O3 -std=c++17 -DZK_MUL_INLINE=1 -fPIC -c $W/$m/zecale_amd/csrc/ntt.hip -o $W/$m/ntt.o &&
      objs=$(cd $ROOT && python3 -c "import __graft_entry__ as g; print(' '.join('build/' + s.rsplit('.', 1)[0] + '.o' for s in g.HIP_SOURCES + g.HOST_SOURCES))" | sed "s#build/ntt\.o#$W/$m/ntt.o#") &&
      cd $ROOT && hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o $W/$m/libzkhip.so $objs && echo "built $m" ) &
  done
  wait
  for m in $MUTANTS; do [ -f $W/$m/libzkhip.so ] || { echo "missing $W/$m/libzkhip.so"; exit 1; }; done
  exit 0
fi

[ "$1" = run ] || { echo "usage: $0 build | run [NAME]"; exit 2; }
[ -n "$2" ] && MUTANTS="$2"
cd $ROOT
OLD="tests/test_ntt_gpu.py"
NEW="tests/test_ntt_layout_gpu.py"
set +e
echo "| mutant | tests/test_ntt_gpu.py | tests/test_ntt_layout_gpu.py |"
echo "|---|---|---|"
for m in $MUTANTS; do
  lib=$W/$m/libzkhip.so
  [ -f $lib ] || { echo "missing $lib"; exit 1; }
  ZKHIP_LIB=$lib timeout -k 10 600 python -m pytest $OLD -x -q -p no:cacheprovider > $W/$m.old.txt 2>&1
  old=$?
  if [ $old -ne 0 ] && [ $old -ne 1 ]; then echo "| $m | exit $old: stopped |  |"; tail -20 $W/$m.old.txt; exit $old; fi
  ZKHIP_LIB=$lib timeout -k 10 600 python -m pytest $NEW -x -q -p no:cacheprovider > $W/$m.new.txt 2>&1
  new=$?
  if [ $new -ne 0 ] && [ $new -ne 1 ]; then echo "| $m | exit $old | exit $new: stopped |"; tail -20 $W/$m.new.txt; exit $new; fi
  verdict() { if [ $1 -eq 1 ]; then echo "killed: $(grep -m1 '^FAILED' $2 | cut -c1-120)"; else echo "survived ($(tail -1 $2 | tr -d '='))"; fi; }
  echo "| $m | $(verdict $old $W/$m.old.txt) | $(verdict $new $W/$m.new.txt) |"
done
