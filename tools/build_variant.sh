#!/bin/bash
# A second build of the library with other compile-time settings, beside the product's:
#   bash tools/build_variant.sh NAME "-DXYZ_INV_THREADS=512 -DXYZ_INV_PREFETCH=1" [file.hip ...]
# -> sperr_amd/libsperr_hip_NAME.so (load it with SPERR_HIP_LIB=...).  Only the named sources (default: the lifting
# units, lift_*.hip, which the XYZ_* switches of lift_xyz.h are for) are compiled with the extra flags; the other
# objects are the product build's.  The units, the flags and the compiler are the Makefile's (SRCS, FLAGS, HIPCC, ARCH).
set -e
name=$1; flags=$2; shift 2
here=$(cd $(dirname $0)/../sperr_amd/csrc && pwd)
mkvar() { make -s --no-print-directory -C $here --eval 'print-%: ; @echo $($*)' print-$1; }
units=$(mkvar SRCS); base=$(mkvar FLAGS); hipcc=$(mkvar HIPCC); arch=$(mkvar ARCH)
srcs=$(echo ${@:-$(for u in $units; do case $u in lift_*) echo $u ;; esac; done)})   # (on one line)
[ -n "$srcs" ] || { echo "no source to compile with $flags" >&2; exit 1; }
for f in $srcs; do
  echo " $units " | grep -q " $f " || { echo "$f is not a unit of the library ($units)" >&2; exit 1; }
done
make -s -C $here
mkdir -p $here/_build/var_$name
objs=""; pids=""
for u in $units; do
  f=${u%.hip}
  if echo " $srcs " | grep -q " $u "; then
    $hipcc $base $flags -c $here/$u -o $here/_build/var_$name/$f.o &
    pids="$pids $!"
    objs="$objs $here/_build/var_$name/$f.o"
  else
    objs="$objs $here/_build/$f.o"
  fi
done
for p in $pids; do wait $p; done
$hipcc --offload-arch=$arch -shared -fPIC -o $here/../libsperr_hip_$name.so $objs
echo "built $here/../libsperr_hip_$name.so (with $flags:" $srcs")"
