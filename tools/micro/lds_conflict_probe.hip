// What does one wave instruction of ds_add_f64 cost when several of its 64 lanes add into the SAME double?
// The fused KKT solve's forward sweep and residual push ~21 lanes of an instruction onto each of two LDS addresses
// (the two expansion columns u, v of a second-order cone); neither vendor guide gives the price.
//
// Shape of the solve launch: 256-thread workgroups, four per CU on all 256 CUs, 32 KB of dynamic LDS each.  The loop
// issues ds_add_f64 of a register value and nothing else (no global traffic, no returning atomics, no barrier).
// Patterns, one address per lane, fixed over the loop:
//   a        64 distinct doubles
//   b        lanes l = 0 (mod 3) on one double, l = 1 (mod 3) on a second, the rest distinct   (forward, level 2)
//   c R      as b, each hot target spread round-robin over R consecutive doubles                (R = 2, 4, 8, 16)
//   d        triples of neighbouring lanes on one double                                        (residual, rows s_j)
//   e        64 lanes on one double
// Output: ns per wave instruction and per CU = kernel time / (16 waves x instructions per wave), best of 3 launches,
// and the same figure in cycles of the shader clock the runtime reports.
//   hipcc --offload-arch=gfx950 -O3 -munsafe-fp-atomics -o lds_conflict_probe tools/micro/lds_conflict_probe.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#define CK(x)                                                                                                          \
    do {                                                                                                               \
        hipError_t e_ = (x);                                                                                           \
        if (e_ != hipSuccess) {                                                                                        \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));                                 \
            exit(2);                                                                                                   \
        }                                                                                                              \
    } while (0)

constexpr int LDS_DOUBLES = 4096; // 32 KB
constexpr int HOT0 = 3000;        // the hot targets and their spread: HOT0 .. HOT0 + 2 * 16 - 1 < LDS_DOUBLES
constexpr int UNROLL = 8;

enum { PAT_A = 0, PAT_B = 1, PAT_C = 2, PAT_D = 3, PAT_E = 4 };

__device__ __forceinline__ int target_of(int pat, int R, int tid) {
    const int lane = tid & 63, own = tid; // own: distinct over the whole workgroup, 0..255
    switch (pat) {
    case PAT_A: return own;
    case PAT_B: return lane % 3 == 0 ? HOT0 : lane % 3 == 1 ? HOT0 + 1 : own;
    case PAT_C: return lane % 3 == 0 ? HOT0 + (lane / 3) % R : lane % 3 == 1 ? HOT0 + R + (lane / 3) % R : own;
    case PAT_D: return (tid >> 6) * 64 + lane / 3;
    default: return HOT0;
    }
}

__global__ __launch_bounds__(256) void k_lds_add(double *out, int pat, int R, int iters) {
    extern __shared__ double lds[];
    for (int i = threadIdx.x; i < LDS_DOUBLES; i += 256) lds[i] = 0.0;
    __syncthreads();
    double *p = &lds[target_of(pat, R, threadIdx.x)];
    const double v = 1.0 + (double)(threadIdx.x & 7);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) atomicAdd(p, v);
    }
    __syncthreads();
    double s = 0.0;
    for (int i = threadIdx.x; i < LDS_DOUBLES; i += 256) s += lds[i];
    out[blockIdx.x * 256 + threadIdx.x] = s; // keeps the adds alive; the host checks the sum
}

int main(int argc, char **argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 2048;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount, wg_per_cu = 4, grid = cus * wg_per_cu;
    const double mhz = prop.clockRate / 1e3;
    int occ = 0;
    CK(hipFuncSetAttribute((const void *)k_lds_add, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_DOUBLES * 8));
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_lds_add, 256, LDS_DOUBLES * 8));
    printf("%s: %d CUs, %.0f MHz, grid %d x 256, %d B LDS, occupancy %d workgroups/CU, %d adds per lane\n", prop.name, cus,
           mhz, grid, LDS_DOUBLES * 8, occ, iters * UNROLL);
    if (occ < wg_per_cu) {
        fprintf(stderr, "the grid would not be co-resident\n");
        return 2;
    }
    double *out, *host = (double *)malloc(sizeof(double) * grid * 256);
    CK(hipMalloc(&out, sizeof(double) * grid * 256));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    struct Case {
        const char *name;
        int pat, R;
    } cases[] = {{"a  64 distinct", PAT_A, 1},      {"b  2 x 21 lanes + 22", PAT_B, 1}, {"c  as b, R = 2", PAT_C, 2},
                 {"c  as b, R = 4", PAT_C, 4},      {"c  as b, R = 8", PAT_C, 8},       {"c  as b, R = 16", PAT_C, 16},
                 {"d  triples of lanes", PAT_D, 1}, {"e  64 lanes on one", PAT_E, 1}};
    const double per_cu = 4.0 * wg_per_cu * (double)iters * UNROLL; // wave instructions per CU and launch
    printf("%-24s %12s %14s %12s\n", "pattern", "launch us", "ns/instr/CU", "cycles");
    int bad = 0;
    for (const Case &c : cases) {
        float best = 1e30f;
        for (int rep = 0; rep < 4; ++rep) { // the first launch warms up
            CK(hipEventRecord(e0));
            k_lds_add<<<grid, 256, LDS_DOUBLES * 8>>>(out, c.pat, c.R, iters);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (rep > 0 && ms < best) best = ms;
        }
        CK(hipMemcpy(host, out, sizeof(double) * grid * 256, hipMemcpyDeviceToHost));
        // every thread of a workgroup holds a partial of the slice's sum; a workgroup's total is 256 lanes x adds x value
        double want = 0.0, got = 0.0;
        for (int t = 0; t < 256; ++t) want += (1.0 + (t & 7)) * (double)iters * UNROLL, got += host[t];
        if (got != want) ++bad;
        const double ns = best * 1e6 / per_cu;
        printf("%-24s %12.1f %14.2f %12.1f%s\n", c.name, best * 1e3, ns, ns * mhz / 1e3, got != want ? "  SUM WRONG" : "");
    }
    CK(hipFree(out));
    free(host);
    return bad ? 1 : 0;
}
