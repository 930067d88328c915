#!/bin/bash
# Mutation record of tests/test_point_ops_gpu.py (profiles/mutation_point_ops.md).  Nine scratch builds of the library, each with ONE
# line of zecale_amd/csrc/ec_mem.cuh or ec_edw.cuh changed.  A mutant changes which multiple of p an fp_sub<K> lends, a neg / F <-> G
# selection, a zero test's value or which coordinate a step takes - never an address outside the operand, a trip count, a vote, a
# barrier or an array bound: it computes wrong values and cannot fault.  Nothing in the tree is modified: the copies are built under $W
# from a copy of the sources, and the tests load them through ZKHIP_LIB.  Two units are recompiled per mutant - msm.hip (every MSM
# kernel: what the old tests run) and point_ops_selftest.hip (the hook: what the new file runs); the tree's other objects are linked in.
#   tools/mutation_point_ops.sh build [-jN]   compile the mutants (CPU only; needs build/*.o from __graft_entry__.build()), N at a time (4)
#   tools/mutation_point_ops.sh run [NAME]    per mutant: the old tests that run the mutated code, then the new file; each under its
#                                             own time limit; one table row per mutant
#   tools/mutation_point_ops.sh base          the same two commands on the tree's own library (times of the unmutated tests)
# `build` STOPS with a message when the line it patches no longer occurs exactly once in its function: the script must follow the source.
# A run stops at the first exit status other than 0 (passed) or 1 (tests failed): the mutant is not run further, nor the next one.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
W=${ZKHIP_MUTANT_DIR:-$ROOT/build/mutants_point}
# (a tenth, edw_dbl_quad_E_lend, is kept in the table below but not in the set: no input can show it - the record proves it.
#  ZKHIP_MUTANTS="edw_dbl_quad_E_lend" tools/mutation_point_ops.sh build, then run, reproduces its row)
MUTANTS=${ZKHIP_MUTANTS:-"madd_mem_P_lend add_lds_regy_QX3_lend madd_lds_regy_R_lend dbl_mem_SX3_lend edw_madd_sel_swapped edw_open_neg_dropped is_zero_rare_drops_p add_quad_q1_q3_swapped from_affine_xe_unchecked"}

mutate() {      # name dir: one exact replacement inside one function (from `anchor` to the function's closing brace)
  python3 - "$1" "$2" <<'EOF'
import sys
name, d = sys.argv[1], sys.argv[2]
M = {
    # file, anchor (occurs once: the function's head), the line, its replacement
    "madd_mem_P_lend": ("ec_mem.cuh", "bool madd_mem(const XyzzRef& acc",
        "case 0: T0 = fp_sub<FqParams, 16>(r, mem_ld(acc, CX)); break;",
        "case 0: T0 = fp_sub<FqParams, 8>(r, mem_ld(acc, CX)); break;"),
    "add_lds_regy_QX3_lend": ("ec_mem.cuh", "bool add_lds_regy(const XyzzRef& spill",
        "T0 = fp_sub<FqParams, 16>(T0, X3);",
        "T0 = fp_sub<FqParams, 8>(T0, X3);"),
    "madd_lds_regy_R_lend": ("ec_mem.cuh", "bool madd_lds_regy(const XyzzRef& acc",
        "case 1: T1 = fp_sub<FqParams, 4>(r, ty); break;",
        "case 1: T1 = fp_sub<FqParams, 2>(r, ty); break;"),
    "dbl_mem_SX3_lend": ("ec_mem.cuh", "void dbl_mem(const XyzzRef& A)",
        "Fq Y3 = fp_mul2(T3, fp_sub<FqParams, 8>(T2, T0), T1,",
        "Fq Y3 = fp_mul2(T3, fp_sub<FqParams, 4>(T2, T0), T1,"),
    "edw_dbl_quad_E_lend": ("ec_edw.cuh", "void edw_dbl_mem_quad(const XyzzRef& A, uint32_t q)",
        "E = fp_sub<FqParams, 4>(xy, H);",
        "E = fp_sub<FqParams, 2>(xy, H);"),
    "edw_madd_sel_swapped": ("ec_edw.cuh", "void edw_madd_lds_regy(uint32_t* xs",
        "case 3: a = T1; b = fq_sel(neg, T3, T2); break;",
        "case 3: a = T1; b = fq_sel(neg, T2, T3); break;"),
    "edw_open_neg_dropped": ("ec_edw.cuh", "void edw_open_lds_pre(uint32_t* xs",
        "if (neg) a = fp_sub_k<FqParams, 1>(fp_zero<FqParams>(), a);",
        "if (neg) a = a;"),
    "is_zero_rare_drops_p": ("ec_mem.cuh", "bool fp_is_zero_2p_rare(const Fq& a)",
        "const bool maybe = (a.l[0] == 0u) | (a.l[0] == FqParams::P[0]);",
        "const bool maybe = (a.l[0] == 0u);"),
    "add_quad_q1_q3_swapped": ("ec_mem.cuh", "void add_mem_quad(const XyzzRef& A, const XyzzRef& B, uint32_t q)",
        "a = odd ? mem_ld_lane(B, q == 1 ? CX : CY) : mem_ld_lane(A, q == 0 ? CX : CY);",
        "a = odd ? mem_ld_lane(B, q == 1 ? CY : CX) : mem_ld_lane(A, q == 0 ? CX : CY);"),
    "from_affine_xe_unchecked": ("ec_edw.cuh", "bool edw_from_affine(const Fq& x, const Fq& y, EdwPacked* out)",
        "const bool ok = on_curve && fq_is_square_nonzero(X) && !fp_is_zero_2p(den) && !fp_is_zero_2p(xe);",
        "const bool ok = on_curve && fq_is_square_nonzero(X) && !fp_is_zero_2p(den);"),
}
fn, anchor, old, new = M[name]
path = d + "/zecale_amd/csrc/" + fn
s = open(path).read()
def stop(what):
    sys.exit("mutation_point_ops.sh: mutant '%s': %s in %s\nupdate the pattern to the source before trusting the record" % (name, what, fn))
if s.count(anchor) != 1:
    stop("the function head occurs %d times, not once:\n    %s\n" % (s.count(anchor), anchor))
a = s.index(anchor)
e = s.index("\n}\n", a)
body = s[a:e]
if body.count(old) != 1:
    stop("the line occurs %d times in its function, not once:\n    %s\n" % (body.count(old), old))
open(path, "w").write(s[:a] + body.replace(old, new) + s[e:])
print("mutated", name)
EOF
}

if [ "$1" = build ]; then
  [ -f $ROOT/build/msm.o ] && [ -f $ROOT/build/point_ops_selftest.o ] || { echo "mutation_point_ops.sh: build the tree first (build/msm.o, build/point_ops_selftest.o)"; exit 1; }
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
    for u in msm point_ops_selftest; do
      ( hipcc $flags -c $W/$m/zecale_amd/csrc/$u.hip -o $W/$m/$u.o && echo "compiled $m/$u" ) &
      n=$((n + 1)); [ $((n % J)) -eq 0 ] && wait
    done
  done
  wait
  for m in $MUTANTS; do
    ( cd $ROOT && hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o $W/$m/libzkhip.so \
        $(echo $objs | sed "s#build/msm\.o#$W/$m/msm.o#; s#build/point_ops_selftest\.o#$W/$m/point_ops_selftest.o#") && echo "built $m" )
  done
  for m in $MUTANTS; do [ -f $W/$m/libzkhip.so ] || { echo "missing $W/$m/libzkhip.so"; exit 1; }; done
  exit 0
fi

[ "$1" = run ] || [ "$1" = base ] || { echo "usage: $0 build [-jN] | run [NAME] | base"; exit 2; }
[ -n "$2" ] && MUTANTS="$2"
[ "$1" = base ] && MUTANTS="unmutated"
cd $ROOT
mkdir -p $W
OLD="tests/test_msm_gpu.py::test_golden_vectors tests/test_msm_edges_gpu.py tests/test_msm_edwards_gpu.py"
NEW="tests/test_point_ops_gpu.py"
set +e
echo "| mutant | old tests | tests/test_point_ops_gpu.py |"
echo "|---|---|---|"
for m in $MUTANTS; do
  lib=$W/$m/libzkhip.so
  [ $m = unmutated ] && lib=$ROOT/zecale_amd/libzkhip.so
  [ -f $lib ] || { echo "missing $lib"; exit 1; }
  ZKHIP_LIB=$lib timeout -k 10 600 python -m pytest $OLD -q -p no:cacheprovider > $W/$m.old.txt 2>&1
  old=$?
  if [ $old -ne 0 ] && [ $old -ne 1 ]; then echo "| $m | exit $old: stopped |  |"; tail -20 $W/$m.old.txt; exit $old; fi
  ZKHIP_LIB=$lib timeout -k 10 300 python -m pytest $NEW -q -p no:cacheprovider --durations=3 > $W/$m.new.txt 2>&1
  new=$?
  if [ $new -ne 0 ] && [ $new -ne 1 ]; then echo "| $m | exit $old | exit $new: stopped |"; tail -20 $W/$m.new.txt; exit $new; fi
  # the failed tests by parameter and, where the messages give them, the counts of failed cases in the same order
  verdict() { if [ $1 -eq 1 ]; then echo "FAILED ($(tail -1 $2 | tr -d '=')): $(grep '^FAILED' $2 | sed -E 's/^FAILED [^:]*:://; s/ - .*//' | tr '\n' ' ' | cut -c1-600) $(grep -oE 'Error: [0-9]+ of [0-9]+ cases failed' $2 | sed 's/Error: //' | tr '\n' ';')"; else echo "passed ($(tail -1 $2 | tr -d '='))"; fi; }
  echo "| $m | $(verdict $old $W/$m.old.txt) | $(verdict $new $W/$m.new.txt) |"
  [ $m = unmutated ] && grep -E "s call" $W/$m.new.txt
done
exit 0
