# Builds the probe beside the repository's other build products (build/ is ignored) and runs it.
#   tools/micro/lds_conflict_probe.sh build        compile only (cross-compiles without a GPU)
#   tools/micro/lds_conflict_probe.sh [ITERS]      compile if needed, run, print the table (keep it under profiles/)
R=$(cd "$(dirname "$0")/../.." && pwd); B=$R/build/micro; mkdir -p $B
if [ ! -x $B/lds_conflict_probe ] || [ $R/tools/micro/lds_conflict_probe.hip -nt $B/lds_conflict_probe ]; then
    hipcc --offload-arch=gfx950 -O3 -munsafe-fp-atomics -o $B/lds_conflict_probe $R/tools/micro/lds_conflict_probe.hip || exit 1
fi
[ "$1" = build ] && exit 0
timeout -k 10 120 $B/lds_conflict_probe "$@"
