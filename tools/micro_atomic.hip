/*
 * micro_atomic — decides the C4 (Q18 150M-group agg) question: does the
 * ~1.8 TB/s random-atomic line ceiling lift when the target table is
 * Infinity-Cache-resident (<= 256 MB)? If yes, partitioning the input by
 * group-key range and building L3-resident sub-tables sequentially would
 * beat the single fused pass; if no, the fused agg is at its true wall.
 *
 *   hipcc --offload-arch=gfx950 -O3 -munsafe-fp-atomics micro_atomic.hip \
 *         -o micro_atomic
 *   ./micro_atomic            the table-size sweep above
 *   ./micro_atomic records    the record-shaped modes below
 *
 * `records` asks the group-join accumulate's question (profiles/README.md
 * Round 7): a 32-B record of 4 u64 takes 3-4 adds per match. Does it cost
 * one memory-side request per atomic INSTRUCTION that touches the record's
 * line, or one per lane? Every mode adds to the same random records, 64 per
 * wave iteration; they differ in which lanes of which instruction carry the
 * record's slots:
 *   a   one lane per record, three u64 atomicAdd instructions (slots 0,2,3)
 *   a+s as a, plus a plain 8-B store to slot 1
 *   b   lanes 4k..4k+3 of ONE u64 atomicAdd address slots 0..3 of record k
 *       (16 records per instruction, 4 instructions per 64 records)
 *   c   2 lanes per record: lanes 2k,2k+1 address slots 0,1 in one
 *       instruction and slots 2,3 in the next (32 records per instruction)
 *   d   lanes 4k one f64 atomicAdd (slot 0), lanes 4k+1..4k+3 one u64
 *       atomicAdd (slots 1..3): the shape the kernel would use
 */
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>

#define HIP_CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { \
    printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); \
    return 1; } } while (0)

__global__ void k_atomic_rmw(unsigned long long *tab, uint64_t mask,
                             int64_t n_ops) {
    uint64_t x = (uint64_t)(blockIdx.x * blockDim.x + threadIdx.x) *
                 0x9E3779B97F4A7C15ull + 12345;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < n_ops; i += stride) {
        x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
        atomicAdd(&tab[x & mask], 1ull);
    }
}

__global__ void k_plain_read(const unsigned long long *tab, uint64_t mask,
                             int64_t n_ops, unsigned long long *sink) {
    uint64_t x = (uint64_t)(blockIdx.x * blockDim.x + threadIdx.x) *
                 0x9E3779B97F4A7C15ull + 777;
    unsigned long long acc = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < n_ops; i += stride) {
        x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
        acc += tab[x & mask];
    }
    if (acc == 0xDEADBEEF) *sink = acc; /* keep the loads alive */
}

/* ---- record-shaped modes ------------------------------------------------ */

enum { M_A = 0, M_AS, M_B, M_C, M_D, M_COUNT };
static const char *const kModeName[M_COUNT] = {"a", "a+s", "b", "c", "d"};

template <int MODE>
__global__ void k_record_rmw(unsigned long long *tab, uint64_t n_rec,
                             int64_t n_ops) {
    uint64_t x = (uint64_t)(blockIdx.x * blockDim.x + threadIdx.x) *
                 0x9E3779B97F4A7C15ull + 4242;
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    /* n_ops is a multiple of the grid: every lane of a wave runs every trip,
     * so the shuffles below always read a live lane */
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < n_ops; i += stride) {
        x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
        /* this lane's record, uniform over [0, n_rec) */
        const uint32_t rec = (uint32_t)(((x >> 32) * n_rec) >> 32);
        if (MODE == M_A || MODE == M_AS) {
            unsigned long long *r = tab + (size_t)rec * 4;
            atomicAdd(r + 0, 1ull);
            if (MODE == M_AS) r[1] = 1ull;
            atomicAdd(r + 2, 1ull);
            atomicAdd(r + 3, 1ull);
        } else if (MODE == M_B || MODE == M_D) {
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const uint32_t rp =
                    (uint32_t)__shfl((int)rec, (lane & ~3) + p, 64);
                unsigned long long *w = tab + (size_t)rp * 4 + (lane & 3);
                if (MODE == M_D && (lane & 3) == 0)
                    atomicAdd((double *)w, 1.0);
                else
                    atomicAdd(w, 1ull);
            }
        } else { /* M_C */
#pragma unroll
            for (int p = 0; p < 2; p++) {
                const uint32_t rp =
                    (uint32_t)__shfl((int)rec, (lane & ~1) + p, 64);
                unsigned long long *w = tab + (size_t)rp * 4 + (lane & 1);
                atomicAdd(w, 1ull);
                atomicAdd(w + 2, 1ull);
            }
        }
    }
}

template <int MODE>
static int time_mode(unsigned long long *tab, uint64_t n_rec, int64_t n_ops,
                     double *grec_s) {
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL(k_record_rmw<MODE>, dim3(4096), dim3(256), 0, 0, tab,
                       n_rec, n_ops / 8); /* warmup */
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipEventRecord(e0));
    hipLaunchKernelGGL(k_record_rmw<MODE>, dim3(4096), dim3(256), 0, 0, tab,
                       n_rec, n_ops);
    HIP_CHECK(hipEventRecord(e1));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    *grec_s = n_ops / (ms * 1e6);
    HIP_CHECK(hipEventDestroy(e0));
    HIP_CHECK(hipEventDestroy(e1));
    return 0;
}

/* every add must have landed: slot totals over the table against the
 * number of records the mode's launches touched */
__global__ void k_slot_totals(const unsigned long long *tab, uint64_t n_rec,
                              unsigned long long *tot) {
    unsigned long long t0 = 0, t2 = 0, t3 = 0;
    double f0 = 0;
    for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
         r < n_rec; r += (uint64_t)gridDim.x * blockDim.x) {
        t0 += tab[r * 4];
        f0 += __builtin_bit_cast(double, tab[r * 4]);
        t2 += tab[r * 4 + 2];
        t3 += tab[r * 4 + 3];
    }
    atomicAdd(&tot[0], t0);
    atomicAdd(&tot[1], t2);
    atomicAdd(&tot[2], t3);
    atomicAdd((double *)&tot[3], f0);
}

static int run_records() {
    const int64_t n_ops = 1LL << 27; /* 128M records per timed launch */
    const int64_t expect = n_ops + n_ops / 8;
    const int64_t sizes_mb[2] = {467, 64};
    unsigned long long *tot;
    HIP_CHECK(hipMalloc(&tot, 32));
    printf("%8s %5s %12s %10s %s\n", "size_MB", "mode", "Grecords/s",
           "vs a", "adds landed");
    for (int64_t mb : sizes_mb) {
        const uint64_t n_rec = ((uint64_t)mb * 1000000) / 32;
        unsigned long long *tab;
        HIP_CHECK(hipMalloc(&tab, n_rec * 32));
        double base = 0;
        for (int m = 0; m < M_COUNT; m++) {
            HIP_CHECK(hipMemset(tab, 0, n_rec * 32));
            HIP_CHECK(hipMemset(tot, 0, 32));
            double g = 0;
            int rc = 1;
            switch (m) {
            case M_A: rc = time_mode<M_A>(tab, n_rec, n_ops, &g); break;
            case M_AS: rc = time_mode<M_AS>(tab, n_rec, n_ops, &g); break;
            case M_B: rc = time_mode<M_B>(tab, n_rec, n_ops, &g); break;
            case M_C: rc = time_mode<M_C>(tab, n_rec, n_ops, &g); break;
            case M_D: rc = time_mode<M_D>(tab, n_rec, n_ops, &g); break;
            }
            if (rc) return 1;
            hipLaunchKernelGGL(k_slot_totals, dim3(1024), dim3(256), 0, 0,
                               tab, n_rec, tot);
            unsigned long long h[4];
            HIP_CHECK(hipMemcpy(h, tot, 32, hipMemcpyDeviceToHost));
            const double f0 = __builtin_bit_cast(double, h[3]);
            const bool ok = h[1] == (unsigned long long)expect &&
                            h[2] == (unsigned long long)expect &&
                            (m == M_D ? f0 == (double)expect
                                      : h[0] == (unsigned long long)expect);
            if (m == M_A) base = g;
            printf("%8lld %5s %12.3f %9.2fx %s\n", (long long)mb,
                   kModeName[m], g, g / base, ok ? "all" : "LOST ADDS");
        }
        HIP_CHECK(hipFree(tab));
    }
    HIP_CHECK(hipFree(tot));
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "records") return run_records();
    const int64_t n_ops = 1LL << 29; /* 512M ops */
    std::vector<int64_t> sizes_mb = {32, 64, 128, 192, 256, 512, 1024,
                                     2048, 4800};
    unsigned long long *sink;
    HIP_CHECK(hipMalloc(&sink, 8));
    printf("%8s %14s %14s %14s %14s\n", "size_MB", "atomic_Gops", "atomic_TBps",
           "read_Gops", "read_TBps");
    for (int64_t mb : sizes_mb) {
        uint64_t words = (uint64_t)mb << 20 >> 3;
        uint64_t mask = 1;
        while ((mask << 1) <= words) mask <<= 1;
        mask -= 1;
        unsigned long long *tab;
        HIP_CHECK(hipMalloc(&tab, (mask + 1) * 8));
        HIP_CHECK(hipMemset(tab, 0, (mask + 1) * 8));
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        /* warmup */
        hipLaunchKernelGGL(k_atomic_rmw, dim3(4096), dim3(256), 0, 0, tab,
                           mask, n_ops / 8);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(k_atomic_rmw, dim3(4096), dim3(256), 0, 0, tab,
                           mask, n_ops);
        HIP_CHECK(hipEventRecord(e1));
        HIP_CHECK(hipEventSynchronize(e1));
        float ms_a = 0;
        HIP_CHECK(hipEventElapsedTime(&ms_a, e0, e1));
        hipLaunchKernelGGL(k_plain_read, dim3(4096), dim3(256), 0, 0, tab,
                           mask, n_ops / 8, sink);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(k_plain_read, dim3(4096), dim3(256), 0, 0, tab,
                           mask, n_ops, sink);
        HIP_CHECK(hipEventRecord(e1));
        HIP_CHECK(hipEventSynchronize(e1));
        float ms_r = 0;
        HIP_CHECK(hipEventElapsedTime(&ms_r, e0, e1));
        double gops_a = n_ops / (ms_a * 1e6);
        double gops_r = n_ops / (ms_r * 1e6);
        printf("%8lld %14.2f %14.2f %14.2f %14.2f\n", (long long)mb,
               gops_a, gops_a * 64 / 1000.0, gops_r, gops_r * 64 / 1000.0);
        HIP_CHECK(hipFree(tab));
        HIP_CHECK(hipEventDestroy(e0));
        HIP_CHECK(hipEventDestroy(e1));
    }
    HIP_CHECK(hipFree(sink));
    return 0;
}
