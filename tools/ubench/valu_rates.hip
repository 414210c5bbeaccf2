// valu_rates.hip -- measure issue rates of the integer instructions the field arithmetic is made of.
// Each kernel runs ITER iterations of 8 independent dependency chains per lane; reports lane-ops/clk/CU.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include "../../triton_vm_amd/csrc/platform.h"
#define ITER 4096
#define CHAINS 8

#define KERNEL(name, body)                                                       \
__global__ void __launch_bounds__(256) name(u64* out, u64 seed) {                 \
    u64 x[CHAINS]; u32 lo[CHAINS], hi[CHAINS];                                    \
    for (int c = 0; c < CHAINS; c++) { x[c] = seed + threadIdx.x * 977 + c * 131; lo[c] = (u32)x[c] | 1; hi[c] = (u32)(x[c] >> 7) | 3; } \
    for (int i = 0; i < ITER; i++) {                                              \
        _Pragma("unroll") for (int c = 0; c < CHAINS; c++) { body }              \
    }                                                                             \
    u64 acc = 0; for (int c = 0; c < CHAINS; c++) acc ^= x[c] + lo[c] + hi[c];    \
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;                             \
}

KERNEL(k_mad_u64_u32, x[c] = (u64)lo[c] * (u32)x[c] + x[c];)
KERNEL(k_mul_lo_u32, lo[c] = lo[c] * hi[c] + 1;)
KERNEL(k_mul_hi_u32, lo[c] = __umulhi(lo[c], hi[c]) | 0x80000001u;)
KERNEL(k_mad_u32_u24, lo[c] = __umul24(lo[c], hi[c]) + 7;)
KERNEL(k_add_u32, lo[c] = lo[c] + hi[c];)
KERNEL(k_add_u64, x[c] = x[c] + (u64)hi[c];)
KERNEL(k_xor_shift, lo[c] = (lo[c] << 3) ^ hi[c];)
__global__ void __launch_bounds__(256) k_fma_f64(u64* out, u64 seed) {
    double x[CHAINS]; for (int c = 0; c < CHAINS; c++) x[c] = (double)(seed + threadIdx.x + c);
    for (int i = 0; i < ITER; i++) { _Pragma("unroll") for (int c = 0; c < CHAINS; c++) x[c] = __builtin_fma(x[c], 1.0000001, 0.5); }
    double a = 0; for (int c = 0; c < CHAINS; c++) a += x[c];
    out[blockIdx.x * blockDim.x + threadIdx.x] = (u64)a;
}
static inline __device__ u64 montyred(u64 lo, u64 hi) { u64 a = lo + (lo << 32); u64 e = a < lo; u64 b = a - (a >> 32) - e; u64 r = hi - b; return hi < b ? r - 0xFFFFFFFFull : r; }
static inline __device__ u64 mulmod(u64 a, u64 b) {
    u32 a0 = a, a1 = a >> 32, b0 = b, b1 = b >> 32; u64 p00 = (u64)a0 * b0; u64 m1 = (u64)a0 * b1 + (p00 >> 32); u64 m2 = (u64)a1 * b0 + (u32)m1;
    return montyred((m2 << 32) | (u32)p00, (u64)a1 * b1 + (m1 >> 32) + (m2 >> 32)); }
KERNEL(k_mulmod, x[c] = mulmod(x[c], x[c] | 5);)
#include "../../triton_vm_amd/csrc/field.h"   // the product's arithmetic (asm Montgomery reduction)
KERNEL(k_bfe_mul, x[c] = bfe_mul(x[c], x[c] | 5);)
KERNEL(k_bfe_add, x[c] = bfe_add(x[c], (u64)hi[c] << 20);)
KERNEL(k_bfe_sub, x[c] = bfe_sub(x[c], (u64)hi[c] << 20);)

// asm-volatile forms (nothing for the compiler to fold): the issue rate of ONE instruction type, 8 independent chains
#define ASM_KERNEL(name, text)                                                        \
__global__ void __launch_bounds__(256) name(u64* out, u64 seed) {                     \
    u32 lo[CHAINS], hi[CHAINS];                                                        \
    for (int c = 0; c < CHAINS; c++) { lo[c] = (u32)(seed + threadIdx.x * 977 + c * 131) | 1; hi[c] = (u32)(seed >> 7) | 3 | c; } \
    for (int i = 0; i < ITER; i++) {                                                   \
        _Pragma("unroll") for (int c = 0; c < CHAINS; c++) asm volatile(text : "+v"(lo[c]) : "v"(hi[c]));  \
    }                                                                                  \
    u64 acc = 0; for (int c = 0; c < CHAINS; c++) acc ^= lo[c];                        \
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;                                  \
}
ASM_KERNEL(k_asm_add_u32, "v_add_u32 %0, %0, %1")
ASM_KERNEL(k_asm_xor_b32, "v_xor_b32 %0, %0, %1")
ASM_KERNEL(k_asm_mov_b32, "v_mov_b32 %0, %1")
ASM_KERNEL(k_asm_add_co, "v_add_co_u32 %0, vcc, %0, %1")
ASM_KERNEL(k_asm_cndmask, "v_cndmask_b32 %0, %0, %1, vcc")
ASM_KERNEL(k_asm_alignbyte, "v_alignbyte_b32 %0, %0, %1, 1")
ASM_KERNEL(k_asm_lshl_add, "v_lshl_add_u32 %0, %0, 3, %1")
__global__ void __launch_bounds__(256) k_asm_mad_u64_u32(u64* out, u64 seed) {
    u64 x[CHAINS]; u32 lo[CHAINS];
    for (int c = 0; c < CHAINS; c++) { x[c] = seed + threadIdx.x * 977 + c * 131; lo[c] = (u32)x[c] | 1; }
    u64 sink;
    for (int i = 0; i < ITER; i++) {
        _Pragma("unroll") for (int c = 0; c < CHAINS; c++) asm volatile("v_mad_u64_u32 %0, %1, %2, %2, %0" : "+v"(x[c]), "=s"(sink) : "v"(lo[c]));
    }
    u64 acc = 0; for (int c = 0; c < CHAINS; c++) acc ^= x[c];
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

// The recombination of tip5.h (ten 22-bit sums -> one word): what does a shift-add cost against the multiply-add it replaces?  These
// run AT THE ROW KERNEL'S OCCUPANCY -- six wavefronts per SIMD: __launch_bounds__(256, 6) caps the registers, and 24 KB of LDS per
// workgroup (of the CU's 160 KB) admits exactly six workgroups of four wavefronts per CU -- and print SIMD cycles per wavefront
// instruction at the clock the device reports next to the rate.  Eight independent chains per lane, as above.
#define ASM_KERNEL6(name, decl, init, fold, text, ...)                                        \
__global__ void __launch_bounds__(256, 6) name(u64* out, u64 seed) {                          \
    extern __shared__ u32 occupancy_pad[];                                                    \
    decl;                                                                                     \
    for (int c = 0; c < CHAINS; c++) { init; }                                                \
    for (int i = 0; i < ITER; i++) {                                                          \
        _Pragma("unroll") for (int c = 0; c < CHAINS; c++) asm volatile(text : __VA_ARGS__);     \
    }                                                                                         \
    u64 acc = 0; for (int c = 0; c < CHAINS; c++) acc ^= fold;                                \
    if (seed == 0xFFFFFFFFFFFFFFFFull) acc += occupancy_pad[threadIdx.x];   /* (never: keeps the LDS allocation) */ \
    out[blockIdx.x * blockDim.x + threadIdx.x] = acc;                                         \
}
#define U32_STATE u32 lo[CHAINS], hi[CHAINS], mid[CHAINS]
#define U32_INIT lo[c] = (u32)(seed + threadIdx.x * 977 + c * 131) | 1; hi[c] = (u32)(seed >> 7) | 3 | c; mid[c] = hi[c] ^ 0x5555u
#define U64_STATE u64 x[CHAINS], z[CHAINS]; u32 lo[CHAINS]; u64 sink
#define U64_INIT x[c] = seed + threadIdx.x * 977 + c * 131; lo[c] = (u32)x[c] | 1; z[c] = 0
ASM_KERNEL6(k6_add_u32, U32_STATE, U32_INIT, lo[c], "v_add_u32 %0, %0, %1", "+v"(lo[c]) : "v"(hi[c]))
ASM_KERNEL6(k6_add_co_u32, U32_STATE, U32_INIT, lo[c], "v_add_co_u32 %0, vcc, %0, %1", "+v"(lo[c]) : "v"(hi[c]) : "vcc")
ASM_KERNEL6(k6_lshl_add_u32, U32_STATE, U32_INIT, lo[c], "v_lshl_add_u32 %0, %1, 8, %0", "+v"(lo[c]) : "v"(hi[c]))
ASM_KERNEL6(k6_add3_u32, U32_STATE, U32_INIT, lo[c], "v_add3_u32 %0, %0, %1, %2", "+v"(lo[c]) : "v"(hi[c]), "v"(mid[c]))
// v_mad_u64_u32 with a live addend (the running sum of a chain) and with a zero one (the first term of a chain: the addend is the
// inline constant 0, the product goes to a fresh pair that the next iteration's multiplier is taken from)
ASM_KERNEL6(k6_mad_u64_u32_live, U64_STATE, U64_INIT, x[c], "v_mad_u64_u32 %0, %1, %2, %2, %0", "+v"(x[c]), "=s"(sink) : "v"(lo[c]))
ASM_KERNEL6(k6_mad_u64_u32_zero, U64_STATE, U64_INIT, x[c], "v_mad_u64_u32 %0, %1, %2, %3, 0", "=v"(x[c]), "=s"(sink) : "v"(lo[c]), "v"((u32)x[c]))

template <class K> void run6(const char* name, K k, double clock_ghz, int n_cus) {
    const int lds = 24 * 1024, wgs = n_cus * 6 * 8;   // eight full rounds of six workgroups per CU
    hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    u64* out; hipMalloc(&out, (size_t)256 * wgs * 8);
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    hipLaunchKernelGGL(k, dim3(wgs), dim3(256), lds, 0, out, 1ull);
    hipDeviceSynchronize();
    float best = 1e30f;
    for (int rep = 0; rep < 5; rep++) {
        hipEventRecord(a); hipLaunchKernelGGL(k, dim3(wgs), dim3(256), lds, 0, out, 2ull); hipEventRecord(b); hipEventSynchronize(b);
        float ms; hipEventElapsedTime(&ms, a, b);
        if (ms < best) best = ms;
    }
    const double wave_insts_per_simd = (double)wgs * 4 / (n_cus * 4) * ITER * CHAINS;   // wavefront instructions each SIMD issues
    printf("%-24s %8.3f ms  %6.2f SIMD-ns per wavefront instruction = %5.2f cycles @%.2f GHz (reported), 6 wavefronts/SIMD\n", name, best,
           best * 1e6 / wave_insts_per_simd, best * 1e6 / wave_insts_per_simd * clock_ghz, clock_ghz);
    hipFree(out);
}
template <class K> void run(const char* name, K k, double ops_per_iter_chain) {
    u64* out; hipMalloc(&out, 256 * 2048 * 8);
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    hipLaunchKernelGGL(k, dim3(2048), dim3(256), 0, 0, out, 1ull);
    hipDeviceSynchronize();
    hipEventRecord(a); hipLaunchKernelGGL(k, dim3(2048), dim3(256), 0, 0, out, 2ull); hipEventRecord(b); hipEventSynchronize(b);
    float ms; hipEventElapsedTime(&ms, a, b);
    double lane_ops = 2048.0 * 256 * ITER * CHAINS * ops_per_iter_chain;
    printf("%-16s %8.3f ms  %8.2f Glane-ops/s  = %6.2f lane-ops/clk/CU @2.4GHz x256CU\n", name, ms, lane_ops / ms / 1e6, lane_ops / (ms * 1e-3) / (2.4e9 * 256));
    hipFree(out);
}
int main() {
    run("mad_u64_u32", k_mad_u64_u32, 1); run("mul_lo_u32", k_mul_lo_u32, 1); run("mul_hi_u32", k_mul_hi_u32, 1);
    run("mad_u32_u24", k_mad_u32_u24, 1); run("add_u32", k_add_u32, 1); run("add_u64", k_add_u64, 1);
    run("xor_shift", k_xor_shift, 1); run("fma_f64", k_fma_f64, 1); run("mulmod(C, r01a)", k_mulmod, 1); run("bfe_mul(field.h)", k_bfe_mul, 1); run("bfe_add(field.h)", k_bfe_add, 1); run("bfe_sub(field.h)", k_bfe_sub, 1);
    run("asm v_add_u32", k_asm_add_u32, 1); run("asm v_xor_b32", k_asm_xor_b32, 1); run("asm v_mov_b32", k_asm_mov_b32, 1);
    run("asm v_add_co_u32", k_asm_add_co, 1); run("asm v_cndmask", k_asm_cndmask, 1); run("asm v_alignbyte", k_asm_alignbyte, 1);
    run("asm v_lshl_add", k_asm_lshl_add, 1); run("asm mad_u64_u32", k_asm_mad_u64_u32, 1);
    hipDeviceProp_t prop; hipGetDeviceProperties(&prop, 0);
    const double ghz = prop.clockRate / 1e6; const int n_cus = prop.multiProcessorCount;
    run6("v_add_u32", k6_add_u32, ghz, n_cus); run6("v_add_co_u32", k6_add_co_u32, ghz, n_cus);
    run6("v_lshl_add_u32", k6_lshl_add_u32, ghz, n_cus); run6("v_add3_u32", k6_add3_u32, ghz, n_cus);
    run6("v_mad_u64_u32 live addend", k6_mad_u64_u32_live, ghz, n_cus); run6("v_mad_u64_u32 zero addend", k6_mad_u64_u32_zero, ghz, n_cus);
    return 0;
}
