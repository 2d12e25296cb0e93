#!/bin/bash
# Interleaved A/B of library builds on the C4 bench: tools/ab.sh <tag> <reps> lib1 lib2 ...
cd "$GRAFT_REPO_ROOT"; export TMPDIR=/tmp
TAG=$1; R=$2; shift 2
O=${ATZ_OUT:-bench_out}/$TAG   # ATZ_OUT: the directory the results go under
mkdir -p $O
for ((i=1;i<=R;i++)); do
  for L in "$@"; do
    n=$(basename $L .so)
    ATZ_LIB=$L timeout -k 10 240 python3 bench.py --full --steps 3 --warmup 1 --no-cpu > $O/$n.$i.json 2> $O/$n.$i.err || exit 1
  done
done
