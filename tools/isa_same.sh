#!/bin/bash
# Compiles every kernel file (csrc/*.hip) to gfx950 assembly in $1 and compares
# it with the assembly in $2, kernel by kernel wherever a kernel sits
# (tools/isa_funcdiff.py: bodies with renumbered local labels, kernel
# descriptors): a behaviour-preserving source change (e.g. removing an
# experiment switch at its default, or moving kernels between files) leaves the
# device code identical.  A file on both sides is compared with its namesake;
# the files on one side only (a split or a merge) are compared as one group.
# Not product code.
out=$1; base=$2; mkdir -p $out
here="$(cd "$(dirname "$0")" && pwd)"
cd "$here/../reed-solomon-novelpoly_amd/csrc"
for src in *.hip; do
  f=${src%.hip}
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-function -munsafe-fp-atomics --cuda-device-only -S -o $out/$f.s $f.hip 2>/dev/null &
done
wait
rc=0
only_new=(); only_base=()
for s in $out/*.s; do
  f=$(basename $s .s)
  if [ ! -f $base/$f.s ]; then only_new+=($s); continue; fi
  if python3 "$here/isa_funcdiff.py" $base/$f.s $s > $out/$f.diff; then echo "same $f"; else echo "DIFF $f"; cat $out/$f.diff; rc=1; fi
done
for s in $base/*.s; do
  [ -f $out/$(basename $s) ] || only_base+=($s)
done
if [ ${#only_new[@]} -gt 0 ] || [ ${#only_base[@]} -gt 0 ]; then
  names="$(basename -a -s .s "${only_base[@]}" | xargs) -> $(basename -a -s .s "${only_new[@]}" | xargs)"
  if python3 "$here/isa_funcdiff.py" "${only_base[@]}" -- "${only_new[@]}" > $out/moved.diff; then echo "same $names"; else echo "DIFF $names"; rc=1; fi
  cat $out/moved.diff
fi
exit $rc
