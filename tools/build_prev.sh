# Build inversekinematicsann_amd/libikhip_prev.so: the library with the csrc/
# sources of git HEAD, for same-box A/B runs against the working tree
# (tools/fab_ab.sh, tools/ann_ab.sh).  The revision is built by its own Makefile,
# so its list of objects and its rules are the ones it was committed with.
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
T=$(mktemp -d /tmp/ikprev.XXXXXX)
trap 'rm -rf $T' EXIT
C=inversekinematicsann_amd/csrc
mkdir -p $T/$C $T/include
REV=${REV:-HEAD}
OUT=${OUT:-libikhip_prev.so}
if [ "$REV" = WORKTREE ]; then  # the working tree's sources (variant builds: EXTRA=-D...)
  cp "$ROOT/include/ikhip.h" $T/include/
  cp "$ROOT"/$C/*.hip "$ROOT"/$C/*.h "$ROOT"/$C/*.cpp "$ROOT"/$C/Makefile $T/$C/
else
  git -C "$ROOT" show $REV:include/ikhip.h > $T/include/ikhip.h
  for f in $(git -C "$ROOT" ls-tree --name-only $REV $C/); do
    git -C "$ROOT" show $REV:$f > $T/$C/$(basename $f)
  done
fi
LIB="$ROOT/inversekinematicsann_amd/$OUT"
make -s -j${JOBS:-8} -C $T/$C HIPCC="/opt/rocm/bin/hipcc $EXTRA" OUT="$LIB" "$LIB"
echo "built $OUT from $REV"
