#!/bin/bash
# Mutation record of tests/test_msm_edges_gpu.py (profiles/mutation_msm_edges.md).  Six scratch builds of the library, each with ONE
# value-only defect in the rare branches of the MSM's group law - a mutant changes which value is written, never an address, a bound,
# a loop trip count or a synchronisation.  Nothing in the tree is modified: the copies are built under $W from a copy of the sources,
# the tree's other objects are linked in, and the tests load them through ZKHIP_LIB.
#   tools/mutation_msm_edges.sh build        compile the mutants (CPU only; needs build/*.o from __graft_entry__.build())
#   tools/mutation_msm_edges.sh run [NAME]   per mutant: the existing suite (test_msm_gpu.py + the synthetic prover test), then the new
#                                            file; each under its own time limit; prints one table row per mutant
# A run stops at the first exit status other than 0 (passed) or 1 (tests failed): the mutant is not run further, nor the next one.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=${ZKHIP_MUTANT_DIR:-$ROOT/build/mutants}
MUTANTS="madd_same_x_writes_inf add_same_x_doubles_on_cancel fixup_inf_l_copies_l sum_lds_inf_never_set accumulate_inf_never_set pair_kind_dbl_as_inf"

mutate() {      # name dir: one exact replacement (the line must occur exactly once)
  python3 - "$1" "$2" <<'EOF'
import sys
name, d = sys.argv[1], sys.argv[2]
M = {
    "madd_same_x_writes_inf": ("ec_mem.cuh",     # madd_same_x: P + P gives O instead of 2P
        "  Fq R = fp_sub<FqParams, 4>(S2, mem_ld(acc, CY));\n  if (fp_is_zero_2p(fp_sqr(R))) {",
        "  Fq R = fp_sub<FqParams, 4>(S2, mem_ld(acc, CY));\n  if (false && fp_is_zero_2p(fp_sqr(R))) {"),
    "add_same_x_doubles_on_cancel": ("ec_mem.cuh",     # add_same_x: P + (-P) gives 2P instead of O
        "  Fq R = fp_sub<FqParams, 2>(S2, S1);\n  if (fp_is_zero_2p(fp_sqr(R))) {",
        "  Fq R = fp_sub<FqParams, 2>(S2, S1);\n  if (true || fp_is_zero_2p(fp_sqr(R))) {"),
    "fixup_inf_l_copies_l": ("msm.hip",     # k_fixup: an infinite L piece is copied instead of F
        "else mem_copy(dst, l_inf ? pf : pl);",
        "else mem_copy(dst, pl);"),
    "sum_lds_inf_never_set": ("msm.hip",     # k_sum_lds: a row that cancels is not marked infinite
        "if (add_lds_regy(dst, xs, zz, zzz, ty, B)) inf = fp_is_zero_2p(lds_ld(zz));",
        "if (add_lds_regy(dst, xs, zz, zzz, ty, B)) inf = false;"),
    "accumulate_inf_never_set": ("msm.hip",     # k_accumulate: a run that cancels is not marked infinite (not reopened)
        "if (madd_lds_regy(acc, xs, zz, zzz, ty, p, neg)) inf = fp_is_zero_2p(lds_ld(zz));",
        "if (madd_lds_regy(acc, xs, zz, zzz, ty, p, neg)) inf = false;"),
    "pair_kind_dbl_as_inf": ("ec_affine.cuh",     # pair_kind_same_x: an affine pair P + P gives O
        "return fp_is_zero_2p(fp_mul(t, fp_one<FqParams>())) ? PK_DBL : PK_INF;",
        "return fp_is_zero_2p(fp_mul(t, fp_one<FqParams>())) ? PK_INF : PK_INF;"),
}
f, old, new = M[name]
p = d + "/" + f
s = open(p).read()
assert s.count(old) == 1, (name, s.count(old))
open(p, "w").write(s.replace(old, new))
print("mutated", name, "in", f)
EOF
}

if [ "$1" = build ]; then
  [ -f $ROOT/build/msm.o ]
  rm -rf $W && mkdir -p $W
  for m in $MUTANTS; do
    mkdir -p $W/$m/include $W/$m/zecale_amd                  # (msm.h includes ../../include/zkhip.h)
    cp -r $ROOT/zecale_amd/csrc $W/$m/zecale_amd/csrc
    cp $ROOT/include/*.h* $W/$m/include/
    mutate $m $W/$m/zecale_amd/csrc
    ( hipcc --offload-arch=gfx950 -O3 -std=c++17 -DZK_MUL_INLINE=1 -fPIC -c $W/$m/zecale_amd/csrc/msm.hip -o $W/$m/msm.o &&
      objs="$W/$m/msm.o $(ls $ROOT/build/*.o | grep -v '/msm\.o$')" &&      # every object of the tree but the one rebuilt here
      hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o $W/$m/libzkhip.so $objs && echo "built $m" ) &
  done
  wait
  for m in $MUTANTS; do [ -f $W/$m/libzkhip.so ] || { echo "missing $W/$m/libzkhip.so"; exit 1; }; done
  exit 0
fi

[ "$1" = run ] || { echo "usage: $0 build | run [NAME]"; exit 2; }
[ -n "$2" ] && MUTANTS="$2"
cd $ROOT
OLD="tests/test_msm_gpu.py tests/test_prover_gpu.py::test_synthetic_circuit_vs_oracle_and_trapdoor"
NEW="tests/test_msm_edges_gpu.py"
set +e
echo "| mutant | existing suite | new tests |"
echo "|---|---|---|"
for m in $MUTANTS; do
  lib=$W/$m/libzkhip.so
  [ -f $lib ] || { echo "missing $lib"; exit 1; }
  ZKHIP_LIB=$lib timeout -k 10 900 python -m pytest $OLD -x -q -p no:cacheprovider > $W/$m.old.txt 2>&1
  old=$?
  if [ $old -ne 0 ] && [ $old -ne 1 ]; then echo "| $m | exit $old: stopped |  |"; tail -20 $W/$m.old.txt; exit $old; fi
  ZKHIP_LIB=$lib timeout -k 10 600 python -m pytest $NEW -x -q -p no:cacheprovider > $W/$m.new.txt 2>&1
  new=$?
  if [ $new -ne 0 ] && [ $new -ne 1 ]; then echo "| $m | exit $old | exit $new: stopped |"; tail -20 $W/$m.new.txt; exit $new; fi
  verdict() { if [ $1 -eq 1 ]; then echo "killed: $(grep -m1 '^FAILED' $2 | cut -c1-110)"; else echo "survived (passed)"; fi; }
  echo "| $m | $(verdict $old $W/$m.old.txt) | $(verdict $new $W/$m.new.txt) |"
done
