#!/bin/bash
# Mutation record of tests/test_field_ops_gpu.py (profiles/mutation_field_ops.md).  Seven scratch builds of the library, each with ONE
# line of zecale_amd/csrc/fp29.cuh, fp_inv.cuh or bw6_params.h changed.  A mutant changes arithmetic or a table entry - never a bound, a
# trip count, a wave vote, a synchronisation or an address.  Nothing in the tree is modified: the copies are built under $W from a copy
# of the sources, and the tests load them through ZKHIP_LIB.  Only msm.hip is recompiled per mutant: it holds both field test hooks and
# every MSM kernel, which is all that the tests named below run; the tree's other objects are linked in as they are.
#   tools/mutation_field_ops.sh build [-jN]   compile the mutants (CPU only; needs build/*.o from __graft_entry__.build()), N at a time (4)
#   tools/mutation_field_ops.sh run [NAME]    per mutant: the old tests (tests/test_field_gpu.py and the MSM's golden vectors), then the
#                                             new file; each under its own time limit; one table row per mutant
# `build` STOPS with a message when a pattern it patches no longer occurs exactly once in its file: the script must follow the source.
# A run stops at the first exit status other than 0 (passed) or 1 (tests failed): the mutant is not run further, nor the next one.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=${ZKHIP_MUTANT_DIR:-$ROOT/build/mutants_field}
MUTANTS="sub3kp_lend subkp_lend subk16_table_lend cond_sub_kp_top_borrow is_zero_drop_p pack_straddle_shift inv_drop_second_add_p"

mutate() {      # name dir: one exact replacement
  python3 - "$1" "$2" <<'EOF'
import sys
name, d = sys.argv[1], sys.argv[2]
M = {
    # (a) fp_sub_sub2's K p lends 2 * 2^29 per limb where a - b - 2c needs 4 * 2^29 (same number, less borrow room)
    "sub3kp_lend": ("fp29.cuh",
        "for (int i = 0; i + 1 < PR::NL; i++) { l[i] += 4u << 29; l[i + 1] -= 4u; }",
        "for (int i = 0; i + 1 < PR::NL; i++) { l[i] += 2u << 29; l[i + 1] -= 2u; }"),
    # (b) fp_sub_k's K p lends nothing: the canonical limbs of K p
    "subkp_lend": ("fp29.cuh",
        "for (int i = 0; i + 1 < PR::NL; i++) { l[i] += 1u << 29; l[i + 1] -= 1u; }",
        "for (int i = 0; i + 1 < PR::NL; i++) { l[i] += 0u << 29; l[i + 1] -= 0u; }"),
    # (c) Fq's SUBK16 table: limb 25 gives its 2^29 back to limb 26 (same number; limb 25 can now go below zero)
    "subk16_table_lend": ("bw6_params.h",
        "0x3ce0ad17u, 0x34127dc0u, 0x0000048au,",
        "0x3ce0ad17u, 0x14127dc0u, 0x0000048bu,"),
    # (d) fp_cond_sub_kp keeps a when the top limbs come out EQUAL, not only when a < K p
    "cond_sub_kp_top_borrow": ("fp29.cuh",
        "borrow = (i + 1 < N) ? (t >> 29) : (t >> 31);",
        "borrow = (i + 1 < N) ? (t >> 29) : ((t - 1) >> 31);"),
    # (e) fp_is_zero_2p forgets that p is zero too
    "is_zero_drop_p": ("fp29.cuh",
        "return z == 0 || e == 0;",
        "return z == 0;"),
    # (f) fp_pack32's third limb of a word lands one bit too high
    "pack_straddle_shift": ("fp29.cuh",
        "if (i + 2 < N && (58 - sh) < 32) v |= (uint64_t)a.l[i + 2] << (58 - sh);",
        "if (i + 2 < N && (58 - sh) < 32) v |= (uint64_t)a.l[i + 2] << (59 - sh);"),
    # (g) fp_inv's tail: no second conditional addition of p after the sign of f is applied
    "inv_drop_second_add_p": ("fp_inv.cuh",
        "  cond_add_p(t);\n  Fp<PR> x;",
        "  Fp<PR> x;"),
}
fn, old, new = M[name]
path = d + "/zecale_amd/csrc/" + fn
s = open(path).read()
if s.count(old) != 1:
    sys.exit("mutation_field_ops.sh: the line of mutant '%s' occurs %d times in %s, not once:\n    %s\nupdate the pattern to the source before trusting the record" % (name, s.count(old), fn, old))
open(path, "w").write(s.replace(old, new))
print("mutated", name)
EOF
}

if [ "$1" = build ]; then
  [ -f $ROOT/build/msm.o ] || { echo "mutation_field_ops.sh: build the tree first (build/msm.o is missing)"; exit 1; }
  J=4; case "$2" in -j*) J=${2#-j};; esac
  rm -rf $W && mkdir -p $W
  for m in $MUTANTS; do
    mkdir -p $W/$m/include $W/$m/zecale_amd                  # (msm.h includes ../../include/zkhip.h)
    cp -r $ROOT/zecale_amd/csrc $W/$m/zecale_amd/csrc
    cp $ROOT/include/*.h* $W/$m/include/
    mutate $m $W/$m
  done
  objs=$(cd $ROOT && python3 -c "import __graft_entry__ as g; print(' '.join('build/' + s.rsplit('.', 1)[0] + '.o' for s in g.HIP_SOURCES + g.HOST_SOURCES))")
  flags=$(cd $ROOT && python3 -c "import __graft_entry__ as g; print(' '.join(g.HIP_FLAGS))")          # the library's normal flags
  n=0
  for m in $MUTANTS; do
    ( hipcc $flags -c $W/$m/zecale_amd/csrc/msm.hip -o $W/$m/msm.o &&
      cd $ROOT && hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o $W/$m/libzkhip.so $(echo $objs | sed "s#build/msm\.o#$W/$m/msm.o#") && echo "built $m" ) &
    n=$((n + 1)); [ $((n % J)) -eq 0 ] && wait
  done
  wait
  for m in $MUTANTS; do [ -f $W/$m/libzkhip.so ] || { echo "missing $W/$m/libzkhip.so"; exit 1; }; done
  exit 0
fi

[ "$1" = run ] || { echo "usage: $0 build [-jN] | run [NAME]"; exit 2; }
[ -n "$2" ] && MUTANTS="$2"
cd $ROOT
OLD="tests/test_field_gpu.py tests/test_msm_gpu.py::test_golden_vectors"
NEW="tests/test_field_ops_gpu.py"
set +e
echo "| mutant | old tests | tests/test_field_ops_gpu.py |"
echo "|---|---|---|"
for m in $MUTANTS; do
  lib=$W/$m/libzkhip.so
  [ -f $lib ] || { echo "missing $lib"; exit 1; }
  ZKHIP_LIB=$lib timeout -k 10 300 python -m pytest $OLD -q -p no:cacheprovider > $W/$m.old.txt 2>&1
  old=$?
  if [ $old -ne 0 ] && [ $old -ne 1 ]; then echo "| $m | exit $old: stopped |  |"; tail -20 $W/$m.old.txt; exit $old; fi
  ZKHIP_LIB=$lib timeout -k 10 300 python -m pytest $NEW -q -p no:cacheprovider > $W/$m.new.txt 2>&1
  new=$?
  if [ $new -ne 0 ] && [ $new -ne 1 ]; then echo "| $m | exit $old | exit $new: stopped |"; tail -20 $W/$m.new.txt; exit $new; fi
  verdict() { if [ $1 -eq 1 ]; then echo "killed ($(tail -1 $2 | tr -d '=')): $(grep '^FAILED' $2 | sed 's/ - .*//; s/^FAILED [^:]*:://' | tr '\n' ' ' | cut -c1-400)"; else echo "survived ($(tail -1 $2 | tr -d '='))"; fi; }
  echo "| $m | $(verdict $old $W/$m.old.txt) | $(verdict $new $W/$m.new.txt) |"
done
