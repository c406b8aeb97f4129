#!/bin/bash
# Builds the shared libraries of this directory for gfx950 (cross-compiles without a GPU).  Usage: [JOBS=N] build.sh
# By convention: the *.hip files here make the core library libdvdgan_hip.so (include/dvdgan_hip.h), and every sub-directory
# <dir> that holds *.hip files makes a library of its own, libdvdgan_hip_<dir>.so with the header include/dvdgan_hip_<dir>.h
# (its objects stay out of build/*.o).  dvd_gan_amd/lib.py's LIBRARIES has one entry for each.
# The extension family beside it: every ../xsrc/<key>/ that holds *.hip files makes ../xsrc/libdvdx_<key>.so with the header
# include/dvdx_<key>.h (lib.py's EXTENSIONS, MORE_EXTENSIONS and ZCR_EXTENSIONS) -- same flags, same .res files, same out-of-date rule; csrc/common.h may be included.
# Every compile also leaves build/<file>.res = hipcc's kernel-resource-usage remarks (registers, spills, scratch per kernel):
# tests/test_abi_cpu.py holds the hot kernels to "no scratch" with it (a dynamically indexed accumulator array once put every
# convolution kernel's accumulators into scratch memory: 3x on the step, invisible to every parity test).
set -e
cd "$(dirname "$0")"
JOBS=${JOBS:-6}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -munsafe-fp-atomics -Wno-unused-result -Wno-unused-value -Rpass-analysis=kernel-resource-usage"
pids=()

# compile_dir <dir>/ <header>: every out-of-date .hip of the directory ("" = this one) joins the pool of $JOBS compiles
compile_dir() {
  local d=$1 h=../../include/$2 f o r
  mkdir -p "${d}build"
  for f in "$d"*.hip; do
    o=${d}build/$(basename "${f%.hip}").o
    r=${o%.o}.res
    if [ ! -f "$o" ] || [ ! -f "$r" ] || [ "$f" -nt "$o" ] || [ common.h -nt "$o" ] || { [[ "$f" == conv_* || "$f" == gru.hip ]] && { [ conv_common.h -nt "$o" ] || [ prof.h -nt "$o" ]; }; } || [ ../../include/dvdgan_hip.h -nt "$o" ] || [ "$h" -nt "$o" ]; then
      ( hipcc $FLAGS -c "$f" -o "$o" 2> "$r.tmp" || { cat "$r.tmp" >&2; rm -f "$o" "$r.tmp"; exit 1; }
        grep -v "remark:\|^ *[0-9]* |\|^ *| *^" "$r.tmp" >&2 || true      # warnings stay visible
        grep "remark:" "$r.tmp" > "$r" || true; rm -f "$r.tmp" ) &
      pids+=($!)
      if [ ${#pids[@]} -ge $JOBS ]; then wait "${pids[0]}"; pids=("${pids[@]:1}"); fi
    fi
  done
}

dirs=()
for d in */; do
  if compgen -G "$d*.hip" > /dev/null; then dirs+=("${d%/}"); fi
done
compile_dir "" dvdgan_hip.h
for d in "${dirs[@]}"; do compile_dir "$d/" "dvdgan_hip_$d.h"; done
xdirs=()
for d in ../xsrc/*/; do
  if compgen -G "$d*.hip" > /dev/null; then xdirs+=("$(basename "$d")"); fi
done
for d in "${xdirs[@]}"; do compile_dir "../xsrc/$d/" "dvdx_$d.h"; done
for p in "${pids[@]}"; do wait "$p"; done
hipcc --offload-arch=gfx950 -shared -fPIC -o libdvdgan_hip.so build/*.o
echo "built $(pwd)/libdvdgan_hip.so"
for d in "${dirs[@]}"; do
  hipcc --offload-arch=gfx950 -shared -fPIC -o "libdvdgan_hip_$d.so" "$d"/build/*.o
  echo "built $(pwd)/libdvdgan_hip_$d.so"
done
for d in "${xdirs[@]}"; do
  hipcc --offload-arch=gfx950 -shared -fPIC -o "../xsrc/libdvdx_$d.so" "../xsrc/$d"/build/*.o
  echo "built $(cd ../xsrc && pwd)/libdvdx_$d.so"
done
