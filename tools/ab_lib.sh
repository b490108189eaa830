# Dev A/B: build a second, complete libyms.so (optionally with extra compiler defines) into tools/bin/
# from csrc/Makefile's own source list (run on the CPU host):
#   bash tools/ab_lib.sh NAME ["-DFOO=0 ..."]   -> tools/bin/libyms_NAME.so  (select with YMS_LIB=...)
# To record a baseline, run it in a checkout of the commit to compare against and keep the .so.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; DEFS=$2
B=$R/tools/bin/build_$NAME
make -C "$R/yolo-ms_amd/csrc" -j"${JOBS:-8}" BUILD="$B" OUT="$R/tools/bin/libyms_$NAME.so" EXTRA_HIPFLAGS="$DEFS"
rm -rf "$B"
echo built tools/bin/libyms_$NAME.so
