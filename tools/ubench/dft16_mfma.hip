// dft16_mfma.hip -- what does a 16-point transform with power-of-two twiddles cost per element as shifts and butterflies on the
// VALU (csrc/ntt_shift.h: ntt_pow2_points<4, true, false>) and as 24 v_mfma_i32_16x16x64_i8 per sixteen transforms plus a
// recombination (csrc/ntt_mfma.h)?  The gate of the matrix-core variants of the LDE's passes 2 and 3.
//
// One process, registers and LDS only: every lane holds 16 words (one group of the shift form; four sets of four words of the
// matrix-core form, i.e. the same number of elements per lane) and transforms them again and again, each result the next input.
// Candidates for where the 24 constant operands (4 VGPRs each) live:
//   (a) set by set, operands from LDS:  24 ds_read_b128 + 12 for the accumulator inputs per set  (Dft16OperandsAt)
//   (d) all 24 operands resident in registers, two wavefronts per SIMD at up to 256 VGPRs     (Dft16OperandsHeld)
// and the floor under every candidate: the 24 matrix instructions of a set alone.  (b) digit pair by digit pair and (c) unwrapped
// positions issue the same 24 (30) matrix instructions per set with MORE vector work: they sit on the same floor and were not built.
// each with the canonical and with the folded recombination, and each also with the fifteen general multiplications of a
// decimation-in-time butterfly group above the lowest (row_ntt_group, L > 0) in front: the VALU work the matrix pipe can run beside.
// Occupancy: workgroups of eight wavefronts as k_lde_pass3_rows<10, 8>, four wavefronts per SIMD (128 VGPRs) -- two for (d).
// Printed: nanoseconds of one SIMD per wavefront-element (one element in each of the 64 lanes).
//
// build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I triton_vm_amd/csrc -mllvm -amdgpu-mfma-vgpr-form \
//             tools/ubench/dft16_mfma.hip -o tools/ubench/bin/dft16_mfma
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#define TVM_MUL_CARRY_FORM 0   // as ntt.hip compiles bfe_mul
#include "ntt_mfma.h"

using namespace tvm;

#define CHECK(e)                                                                        \
    do {                                                                                \
        hipError_t err_ = (e);                                                          \
        if (err_ != hipSuccess) {                                                       \
            std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(err_)); \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

static __device__ const Dft16MfmaTable d_table = dft16_make_mfma_table(Pow2Root<4, false>::value, dft16_layout_dit());

enum Form { SHIFT, AT_LDS, HELD, PIPE_ONLY };   // PIPE_ONLY: the 24 matrix instructions of a set on resident operands and nothing else

template <Form FORM, bool CANONICAL, bool TWIDDLES, int WAVES_PER_SIMD>
__global__ void __launch_bounds__(512, WAVES_PER_SIMD) k_groups(u64* __restrict__ out, const u64* __restrict__ tw_in, int n_iter) {
    __shared__ __attribute__((aligned(16))) u32 tab_words[sizeof(Dft16MfmaTable) / 4];
    const int tid = threadIdx.x, lane = tid & 63;
    if constexpr (FORM != SHIFT) {
        const u32* src = (const u32*)&d_table;
        for (int i = tid; i < (int)(sizeof(Dft16MfmaTable) / 4); i += blockDim.x) tab_words[i] = src[i];
        __syncthreads();
    }
    const Dft16MfmaTable* table = (const Dft16MfmaTable*)tab_words;
    u64 x[16], tw[4];
#pragma unroll
    for (int e = 0; e < 16; e++) x[e] = ((u64)(blockIdx.x * 512 + tid) * 0x9E3779B97F4A7C15ull + e) >> 1;
#pragma unroll
    for (int e = 0; e < 4; e++) tw[e] = TWIDDLES ? tw_in[(lane + e) & 63] : 0;   // (four, loaded once: the twiddles' own traffic and registers are not what is measured)
    Dft16OperandsHeld held;
    if constexpr (FORM == HELD || FORM == PIPE_ONLY) held.load(table, lane);
    for (int it = 0; it < n_iter; it++) {
        if constexpr (TWIDDLES) {
#pragma unroll
            for (int e = 1; e < 16; e++) x[e] = bfe_mul(x[e], tw[e & 3]);
        }
        if constexpr (FORM == SHIFT) {
            ntt_pow2_points<4, true, false>(x);
        } else {
#pragma unroll
            for (int set = 0; set < 4; set++) {
                u64(&xs)[4] = *reinterpret_cast<u64(*)[4]>(&x[4 * set]);
                if constexpr (FORM == PIPE_ONLY) {
                    // the floor of the matrix pipe: 24 instructions into ONE accumulator (a chain of this shape runs at the issue rate), no
                    // recombination -- four exclusive-ors keep the result alive
                    tvm_v4i lo, hi, acc = held.c(0);
#pragma unroll
                    for (int t = 0; t < 4; t++) lo[t] = (int)(u32)xs[t], hi[t] = (int)(u32)(xs[t] >> 32);
#pragma unroll
                    for (int d = 0; d < DFT16_MFMA_DIGITS; d++) acc = TVM_MFMA_I8(held.a(d, 1), hi, TVM_MFMA_I8(held.a(d, 0), lo, acc));
#pragma unroll
                    for (int t = 0; t < 4; t++) xs[t] ^= (u64)(u32)acc[t] << (8 * t);
                } else if constexpr (FORM == HELD) dft16_mfma<CANONICAL>(xs, held);
                else dft16_mfma<CANONICAL>(xs, Dft16OperandsAt{table, tvm_opaque(lane)});   // (opaque: the operands are fetched again for every set, not hoisted out of the loop and spilled)
            }
        }
    }
    u64 acc = 0;
#pragma unroll
    for (int e = 0; e < 16; e++) acc ^= x[e];
    out[(u64)blockIdx.x * 512 + tid] = acc;
}

template <Form FORM, bool CANONICAL, bool TWIDDLES, int WAVES_PER_SIMD>
double run(const char* name, int n_cus, const u64* tw) {
    const int resident = WAVES_PER_SIMD / 2;                   // workgroups of eight wavefronts per CU
    const int workgroups = n_cus * resident * 8, n_iter = 256;
    u64* out;
    CHECK(hipMalloc(&out, (size_t)workgroups * 512 * 8));
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    // two (four) wavefronts per SIMD means ONE workgroup (two) per CU whatever the registers allow: dynamic LDS nobody touches takes the room of another
    const size_t dyn_lds = WAVES_PER_SIMD == 2 ? 84 * 1024 : 54 * 1024;   // (four per SIMD: two workgroups per CU with or without the 25 KB table, never three)
    CHECK(hipFuncSetAttribute((const void*)k_groups<FORM, CANONICAL, TWIDDLES, WAVES_PER_SIMD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_lds));
    auto launch = [&] { hipLaunchKernelGGL((k_groups<FORM, CANONICAL, TWIDDLES, WAVES_PER_SIMD>), dim3(workgroups), dim3(512), dyn_lds, 0, out, tw, n_iter); };
    launch();   // warm-up
    CHECK(hipDeviceSynchronize());
    double best = 1e30;
    for (int rep = 0; rep < 5; rep++) {
        CHECK(hipEventRecord(a));
        launch();
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        float ms;
        CHECK(hipEventElapsedTime(&ms, a, b));
        if (ms < best) best = ms;
    }
    CHECK(hipGetLastError());
    CHECK(hipFree(out));
    const double wave_elements = (double)workgroups * 8 * n_iter * 16;
    const double ns = best * 1e6 * (4.0 * n_cus) / wave_elements;
    std::printf("  %-66s %8.3f ms   %7.2f SIMD-ns per wavefront-element\n", name, best, ns);
    return ns;
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int n_cus = prop.multiProcessorCount;
    std::printf("device: %s, %d CUs, clock %d MHz (reported)\n", prop.name, n_cus, prop.clockRate / 1000);
    u64 h_tw[64], *tw;
    for (int i = 0; i < 64; i++) h_tw[i] = (0x9E3779B97F4A7C15ull * (i + 1)) >> 1;
    CHECK(hipMalloc(&tw, sizeof(h_tw)));
    CHECK(hipMemcpy(tw, h_tw, sizeof(h_tw), hipMemcpyHostToDevice));
    std::printf("registers and LDS only, workgroups of 512 work-items, 256 transforms of 16 words per lane, best of 5:\n");
    std::printf("the 16-point transform alone\n");
    const double s4 = run<SHIFT, true, false, 4>("shift form, 4 wavefronts per SIMD", n_cus, tw);
    const double s2 = run<SHIFT, true, false, 2>("shift form, 2 wavefronts per SIMD", n_cus, tw);
    const double ac = run<AT_LDS, true, false, 4>("(a) matrix cores, operands from LDS, canonical, 4 per SIMD", n_cus, tw);
    const double af = run<AT_LDS, false, false, 4>("(a) matrix cores, operands from LDS, folded, 4 per SIMD", n_cus, tw);
    const double dc = run<HELD, true, false, 2>("(d) matrix cores, operands in registers, canonical, 2 per SIMD", n_cus, tw);
    const double df = run<HELD, false, false, 2>("(d) matrix cores, operands in registers, folded, 2 per SIMD", n_cus, tw);
    const double p2 = run<PIPE_ONLY, true, false, 2>("the 24 matrix instructions of a set alone (no recombination), 2 per SIMD", n_cus, tw);
    std::printf("  -> one v_mfma_i32_16x16x64_i8 = %.1f SIMD-ns (%.1f cycles at the reported clock); the matrix pipe alone is %.0f %% of the better shift form\n",
                p2 * 4 / 24, p2 * 4 / 24 * prop.clockRate / 1e6, p2 / (s4 < s2 ? s4 : s2) * 100);
    std::printf("the group of a decimation-in-time layer above the lowest: 15 general multiplications + the transform\n");
    const double ts4 = run<SHIFT, true, true, 4>("shift form, 4 per SIMD", n_cus, tw);
    const double ts2 = run<SHIFT, true, true, 2>("shift form, 2 per SIMD", n_cus, tw);
    const double taf = run<AT_LDS, false, true, 4>("(a) operands from LDS, folded, 4 per SIMD", n_cus, tw);
    const double tac = run<AT_LDS, true, true, 4>("(a) operands from LDS, canonical, 4 per SIMD", n_cus, tw);
    const double tdf = run<HELD, false, true, 2>("(d) operands in registers, folded, 2 per SIMD", n_cus, tw);
    const double best_shift = s4 < s2 ? s4 : s2, best_tw_shift = ts4 < ts2 ? ts4 : ts2;
    auto pct = [](double v, double ref) { return (1 - v / ref) * 100; };
    std::printf("against the better shift form: transform alone (a) canonical %+.1f %%, (a) folded %+.1f %%, (d) canonical %+.1f %%, (d) folded %+.1f %%\n",
                pct(ac, best_shift), pct(af, best_shift), pct(dc, best_shift), pct(df, best_shift));
    std::printf("                               group with multiplications (a) folded %+.1f %%, (a) canonical %+.1f %%, (d) folded %+.1f %%   (positive: faster)\n",
                pct(taf, best_tw_shift), pct(tac, best_tw_shift), pct(tdf, best_tw_shift));
    CHECK(hipFree(tw));
    return 0;
}
