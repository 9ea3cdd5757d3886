#!/bin/bash
# Builds libmuopdb_hip.so for gfx950 (hipcc cross-compiles without a GPU).
# -ffp-contract=off: the exact-association distance code must never be contracted into FMAs.
set -e
cd "$(dirname "$0")"
OUT=../libmuopdb_hip.so
SRCS="mdb_core.hip mdb_flat.hip mdb_flat_mfma.hip mdb_ef.hip mdb_ivf.hip mdb_hnsw.hip mdb_hnsw_upper.hip mdb_spann.hip mdb_kmeans.hip mdb_hnsw_build.hip"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unused-variable $MDB_EXTRA_FLAGS"
mkdir -p build
objs=""
pids=""
for s in $SRCS; do
  [ -f "$s" ] || continue
  o=build/${s%.hip}.o
  stale=0
  for h in *.h ../../include/muopdb_hip.h build.sh; do [ "$h" -nt "$o" ] && stale=1; done
  if [ ! -f "$o" ] || [ "$s" -nt "$o" ] || [ $stale = 1 ]; then
    echo "hipcc $s"
    rm -f "$o"   # a failed compile must never leave a stale object for the link step
    # mdb_hnsw.hip: its traversal kernels are ONE wave's dependent instruction chain, not a throughput loop — the ILP-first
    # pre-RA strategy and no post-RA rescheduling measure 4.6 % faster on the headline (0.957 vs 1.003 ms); the same
    # flags slow the streaming kernels of the other files (PQ scan +40 %), so they stay per file
    extra=""
    { [ "$s" = mdb_hnsw.hip ] || [ "$s" = mdb_hnsw_upper.hip ]; } && extra="-mllvm -amdgpu-sched-strategy=max-ilp -mllvm -enable-post-misched=0"
    hipcc $FLAGS $extra -c "$s" -o "$o" &
    pids="$pids $!"
  fi
  objs="$objs $o"
done
# the loaders' host halves (mdb_files.cpp): plain C++, no HIP header — the same file tests/host/check_files_main.cpp builds with the sanitizers
o=build/mdb_files.o
if [ ! -f "$o" ] || [ mdb_files.cpp -nt "$o" ] || [ mdb_files.h -nt "$o" ] || [ ../../include/muopdb_hip.h -nt "$o" ] || [ build.sh -nt "$o" ]; then
  echo "g++ mdb_files.cpp"
  rm -f "$o"
  g++ -std=c++17 -O2 -fPIC -Wall -c mdb_files.cpp -o "$o" &
  pids="$pids $!"
fi
objs="$objs $o"
for p in $pids; do wait "$p" || { echo "build.sh: a translation unit failed to compile" >&2; exit 1; }; done
hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT $objs
echo "built $OUT"
# C++ host mirror demo (include/muopdb_host.hpp over the C ABI; plain g++, no HIP headers needed)
g++ -std=c++17 -O2 -Wall -I../../include ../../examples/host_mirror_demo.cpp -o ../host_mirror_demo \
  -L.. -lmuopdb_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,/opt/rocm/lib
g++ -std=c++17 -O2 -Wall -I../../include ../../examples/replay_search.cpp -o ../replay_search \
  -L.. -lmuopdb_hip -Wl,-rpath,'$ORIGIN' -Wl,-rpath,/opt/rocm/lib
echo "built ../host_mirror_demo ../replay_search"
