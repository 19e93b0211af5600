#!/bin/bash
# Build container: bash tools/build_variant.sh <name> <-D flags...>  ->  inf560-approximate-pattern-matching_amd/libapm_var_<name>.so
# An A/B build of the library that differs from the product in the compile-time knobs of the sieve + verify units only
# (apm_sieve.hip, apm_sieve_diag.hip, apm_verify.hip, counting and record build; the other objects are the product's, the list is the
# Makefile's); picked up on the GPU box through APM_LIB_PATH (tools/ab_libs.sh).  Never shipped.
set -e
NAME=$1; shift
P=$(dirname "$0")/../inf560-approximate-pattern-matching_amd
make -s -C "$P" lib
HIPCC=$(make -s -C "$P" print-HIPCC); HIPFLAGS=$(make -s -C "$P" print-HIPFLAGS); OBJS=$(make -s -C "$P" print-LIB_OBJS)
for u in apm_sieve apm_sieve_diag apm_verify; do
  for rec in "" _rec; do
    $HIPCC $HIPFLAGS ${rec:+-DAPM_REC} "$@" -c "$P/csrc/$u.hip" -o "$P/csrc/$u$rec.var_$NAME.o"
    OBJS=${OBJS/csrc\/$u$rec.o/csrc\/$u$rec.var_$NAME.o}
  done
done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$P/libapm_var_$NAME.so" $OBJS -ldl -lpthread
rm -f "$P"/csrc/*.var_$NAME.o
echo "built libapm_var_$NAME.so"
