#!/bin/bash
# Builds libsdm_hip.so (gfx950) next to the Python package.  hipcc cross-compiles without a GPU.
set -euo pipefail
cd "$(dirname "$0")"
OUT=../libsdm_hip.so
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function"
# --force: recompile every translation unit (what __graft_entry__.build() asks for, so that the
# driver's build check really exercises hipcc); default: only what is older than its sources
[ "${1:-}" = "--force" ] && rm -f ./*.o
objs=()
pids=()
for f in ctx index collisions fused displacement calib comm condensation condensation_formulae parcel parcel_chem parcel_coal freezing deposition chemistry seeding relaxed_velocity initialisation; do
  stale=0
  [ -f $f.o ] || stale=1
  for dep in $f.hip common.h sdm_math.h sdm_math_tables.h physics.h index.h shuffle_device.h shuffle_build.h pair_all_sort_body.inc pair_tag.h collision_pairs.h breakup_pairs.h freezing_rows.h deposition_rows.h ../../include/sdm_parcel_ice.h ../../include/sdm_hip.h ../../include/sdm_condensation.h ../../include/sdm_condensation_formulae.h ../../include/sdm_freezing.h ../../include/sdm_deposition.h ../../include/sdm_chemistry.h ../../include/sdm_seeding.h ../../include/sdm_relaxed_velocity.h ../../include/sdm_initialisation.h ../../include/sdm_parcel.h ../../include/sdm_parcel_diag.h ../../include/sdm_parcel_chem.h ../../include/sdm_parcel_vent.h ../../include/sdm_parcel_coal.h ../../include/sdm_parcel_breakup.h chemistry_rows.h toms748.h condensation_solver.h condensation_formulae.h parcel_solver.h; do
    [ $stale = 1 ] || { [ $dep -nt $f.o ] && stale=1; } || true
  done
  if [ $stale = 1 ]; then
    rm -f $f.o
    $HIPCC $FLAGS -c $f.hip -o $f.o &
    pids+=($!)
  fi
  objs+=($f.o)
done
for pid in "${pids[@]:-}"; do
  [ -z "$pid" ] || wait "$pid"
done
rm -f $OUT
$HIPCC --offload-arch=gfx950 -shared -fPIC -Wl,--no-undefined -o $OUT "${objs[@]}" -ldl
echo "built $(realpath $OUT)"
# the C-ABI example embeds the header's struct layouts: rebuild it with the library
bash ../../examples/build.sh
