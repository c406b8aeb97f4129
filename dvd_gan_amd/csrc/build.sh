#!/bin/bash
# Builds libdvdgan_hip.so, libdvdgan_hip_adv.so, libdvdgan_hip_eval.so, libdvdgan_hip_prdc.so, libdvdgan_hip_aug.so, libdvdgan_hip_geom.so and libdvdgan_hip_sv.so for gfx950 (cross-compiles without a GPU).  Usage: build.sh [-j N]
# Every compile also leaves build/<file>.res = hipcc's kernel-resource-usage remarks (registers, spills, scratch per kernel):
# tests/test_abi_cpu.py holds the hot kernels to "no scratch" with it (a dynamically indexed accumulator array once put every
# convolution kernel's accumulators into scratch memory: 3x on the step, invisible to every parity test).
set -e
cd "$(dirname "$0")"
JOBS=${JOBS:-6}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -munsafe-fp-atomics -Wno-unused-result -Wno-unused-value -Rpass-analysis=kernel-resource-usage"
mkdir -p build
pids=()
for f in *.hip; do
  o=build/${f%.hip}.o
  r=build/${f%.hip}.res
  if [ ! -f "$o" ] || [ ! -f "$r" ] || [ "$f" -nt "$o" ] || [ common.h -nt "$o" ] || { [[ "$f" == conv_* || "$f" == gru.hip ]] && { [ conv_common.h -nt "$o" ] || [ prof.h -nt "$o" ]; }; } || [ ../../include/dvdgan_hip.h -nt "$o" ]; then
    ( hipcc $FLAGS -c "$f" -o "$o" 2> "$r.tmp" || { cat "$r.tmp" >&2; rm -f "$o" "$r.tmp"; exit 1; }
      grep -v "remark:\|^ *[0-9]* |\|^ *| *^" "$r.tmp" >&2 || true      # warnings stay visible
      grep "remark:" "$r.tmp" > "$r" || true; rm -f "$r.tmp" ) &
    pids+=($!)
    if [ ${#pids[@]} -ge $JOBS ]; then wait "${pids[0]}"; pids=("${pids[@]:1}"); fi
  fi
done
for p in "${pids[@]}"; do wait "$p"; done
hipcc --offload-arch=gfx950 -shared -fPIC -o libdvdgan_hip.so build/*.o
echo "built $(pwd)/libdvdgan_hip.so"
# libdvdgan_hip_adv.so (include/dvdgan_hip_adv.h): a library of its own, so its objects stay out of build/*.o
mkdir -p adv/build
for f in adv/*.hip; do
  o=adv/build/$(basename "${f%.hip}").o
  r=adv/build/$(basename "${f%.hip}").res
  if [ ! -f "$o" ] || [ ! -f "$r" ] || [ "$f" -nt "$o" ] || [ common.h -nt "$o" ] || [ ../../include/dvdgan_hip.h -nt "$o" ] || [ ../../include/dvdgan_hip_adv.h -nt "$o" ]; then
    hipcc $FLAGS -c "$f" -o "$o" 2> "$r.tmp" || { cat "$r.tmp" >&2; rm -f "$o" "$r.tmp"; exit 1; }
    grep -v "remark:\|^ *[0-9]* |\|^ *| *^" "$r.tmp" >&2 || true
    grep "remark:" "$r.tmp" > "$r" || true; rm -f "$r.tmp"
  fi
done
hipcc --offload-arch=gfx950 -shared -fPIC -o libdvdgan_hip_adv.so adv/build/*.o
echo "built $(pwd)/libdvdgan_hip_adv.so"
# libdvdgan_hip_eval.so (include/dvdgan_hip_eval.h): the third library, built the same way
mkdir -p eval/build
for f in eval/*.hip; do
  o=eval/build/$(basename "${f%.hip}").o
  r=eval/build/$(basename "${f%.hip}").res
  if [ ! -f "$o" ] || [ ! -f "$r" ] || [ "$f" -nt "$o" ] || [ common.h -nt "$o" ] || [ ../../include/dvdgan_hip.h -nt "$o" ] || [ ../../include/dvdgan_hip_eval.h -nt "$o" ]; then
    hipcc $FLAGS -c "$f" -o "$o" 2> "$r.tmp" || { cat "$r.tmp" >&2; rm -f "$o" "$r.tmp"; exit 1; }
    grep -v "remark:\|^ *[0-9]* |\|^ *| *^" "$r.tmp" >&2 || true
    grep "remark:" "$r.tmp" > "$r" || true; rm -f "$r.tmp"
  fi
done
hipcc --offload-arch=gfx950 -shared -fPIC -o libdvdgan_hip_eval.so eval/build/*.o
echo "built $(pwd)/libdvdgan_hip_eval.so"
# libdvdgan_hip_prdc.so (include/dvdgan_hip_prdc.h): the fourth library, built the same way
mkdir -p prdc/build
for f in prdc/*.hip; do
  o=prdc/build/$(basename "${f%.hip}").o
  r=prdc/build/$(basename "${f%.hip}").res
  if [ ! -f "$o" ] || [ ! -f "$r" ] || [ "$f" -nt "$o" ] || [ common.h -nt "$o" ] || [ ../../include/dvdgan_hip.h -nt "$o" ] || [ ../../include/dvdgan_hip_prdc.h -nt "$o" ]; then
    hipcc $FLAGS -c "$f" -o "$o" 2> "$r.tmp" || { cat "$r.tmp" >&2; rm -f "$o" "$r.tmp"; exit 1; }
    grep -v "remark:\|^ *[0-9]* |\|^ *| *^" "$r.tmp" >&2 || true
    grep "remark:" "$r.tmp" > "$r" || true; rm -f "$r.tmp"
  fi
done
hipcc --offload-arch=gfx950 -shared -fPIC -o libdvdgan_hip_prdc.so prdc/build/*.o
echo "built $(pwd)/libdvdgan_hip_prdc.so"
# libdvdgan_hip_aug.so (include/dvdgan_hip_aug.h): the fifth library, built the same way
mkdir -p aug/build
for f in aug/*.hip; do
  o=aug/build/$(basename "${f%.hip}").o
  r=aug/build/$(basename "${f%.hip}").res
  if [ ! -f "$o" ] || [ ! -f "$r" ] || [ "$f" -nt "$o" ] || [ common.h -nt "$o" ] || [ ../../include/dvdgan_hip.h -nt "$o" ] || [ ../../include/dvdgan_hip_aug.h -nt "$o" ]; then
    hipcc $FLAGS -c "$f" -o "$o" 2> "$r.tmp" || { cat "$r.tmp" >&2; rm -f "$o" "$r.tmp"; exit 1; }
    grep -v "remark:\|^ *[0-9]* |\|^ *| *^" "$r.tmp" >&2 || true
    grep "remark:" "$r.tmp" > "$r" || true; rm -f "$r.tmp"
  fi
done
hipcc --offload-arch=gfx950 -shared -fPIC -o libdvdgan_hip_aug.so aug/build/*.o
echo "built $(pwd)/libdvdgan_hip_aug.so"
# libdvdgan_hip_geom.so (include/dvdgan_hip_geom.h): the sixth library, built the same way
mkdir -p geom/build
for f in geom/*.hip; do
  o=geom/build/$(basename "${f%.hip}").o
  r=geom/build/$(basename "${f%.hip}").res
  if [ ! -f "$o" ] || [ ! -f "$r" ] || [ "$f" -nt "$o" ] || [ common.h -nt "$o" ] || [ ../../include/dvdgan_hip.h -nt "$o" ] || [ ../../include/dvdgan_hip_geom.h -nt "$o" ]; then
    hipcc $FLAGS -c "$f" -o "$o" 2> "$r.tmp" || { cat "$r.tmp" >&2; rm -f "$o" "$r.tmp"; exit 1; }
    grep -v "remark:\|^ *[0-9]* |\|^ *| *^" "$r.tmp" >&2 || true
    grep "remark:" "$r.tmp" > "$r" || true; rm -f "$r.tmp"
  fi
done
hipcc --offload-arch=gfx950 -shared -fPIC -o libdvdgan_hip_geom.so geom/build/*.o
echo "built $(pwd)/libdvdgan_hip_geom.so"
# libdvdgan_hip_sv.so (include/dvdgan_hip_sv.h): the seventh library, built the same way
mkdir -p sv/build
for f in sv/*.hip; do
  o=sv/build/$(basename "${f%.hip}").o
  r=sv/build/$(basename "${f%.hip}").res
  if [ ! -f "$o" ] || [ ! -f "$r" ] || [ "$f" -nt "$o" ] || [ common.h -nt "$o" ] || [ ../../include/dvdgan_hip.h -nt "$o" ] || [ ../../include/dvdgan_hip_sv.h -nt "$o" ]; then
    hipcc $FLAGS -c "$f" -o "$o" 2> "$r.tmp" || { cat "$r.tmp" >&2; rm -f "$o" "$r.tmp"; exit 1; }
    grep -v "remark:\|^ *[0-9]* |\|^ *| *^" "$r.tmp" >&2 || true
    grep "remark:" "$r.tmp" > "$r" || true; rm -f "$r.tmp"
  fi
done
hipcc --offload-arch=gfx950 -shared -fPIC -o libdvdgan_hip_sv.so sv/build/*.o
echo "built $(pwd)/libdvdgan_hip_sv.so"
