// Throughput of the three-input XOR a Philox round needs (hi ^ c ^ k), on one MI355X (gfx950): one v_bitop3_b32 (truth table
// 0x96) against one and two v_xor_b32, with the key in a scalar register as trc_philox4x32_10 has it.
// build: hipcc -O3 --offload-arch=gfx950 -o bitop3 bitop3.hip ; run: ./bitop3
// Each kernel runs ITER x 8 independent chains of one instruction form per lane, 8 waves per SIMD on every CU; the result is
// printed as cycles per wave-instruction per SIMD at 2.4 GHz (see intmul.hip: 2 = the float32 rate with several waves).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#define ITER 4096
#define DEF(NAME, ASM, NI)                                                                            \
__global__ __launch_bounds__(512) void NAME(uint32_t *out, uint32_t seed) {                          \
    uint32_t a0 = threadIdx.x + seed, a1 = a0 * 3u + 1u, a2 = a0 ^ 0x55u, a3 = a0 + 7u,               \
             a4 = a0 * 5u, a5 = a0 + 11u, a6 = a0 ^ 0x77u, a7 = a0 + 13u;                             \
    const uint32_t b = threadIdx.x * 0x9E3779B9u, K = 0xBB67AE85u + seed;                             \
    for (int i = 0; i < ITER; ++i) {                                                                  \
        asm volatile(ASM : "+v"(a0) : "v"(b), "s"(K));                                                \
        asm volatile(ASM : "+v"(a1) : "v"(b), "s"(K));                                                \
        asm volatile(ASM : "+v"(a2) : "v"(b), "s"(K));                                                \
        asm volatile(ASM : "+v"(a3) : "v"(b), "s"(K));                                                \
        asm volatile(ASM : "+v"(a4) : "v"(b), "s"(K));                                                \
        asm volatile(ASM : "+v"(a5) : "v"(b), "s"(K));                                                \
        asm volatile(ASM : "+v"(a6) : "v"(b), "s"(K));                                                \
        asm volatile(ASM : "+v"(a7) : "v"(b), "s"(K));                                                \
    }                                                                                                 \
    out[blockIdx.x * blockDim.x + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;              \
}                                                                                                     \
static const int NAME##_ni = NI;
DEF(k_xor1, "v_xor_b32 %0, %2, %0", 1)
DEF(k_xor2, "v_xor_b32 %0, %1, %0\n\tv_xor_b32 %0, %2, %0", 2)
DEF(k_bitop3, "v_bitop3_b32 %0, %0, %1, %2 bitop3:0x96", 1)

template <class K> static float run(const char *name, K kern, int ni, uint32_t *d) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    const int blocks = 256 * 4;          // 4 x 512 threads per CU = 8 waves per SIMD
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(512), 0, 0, d, 1u);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    for (int r = 0; r < 5; ++r) hipLaunchKernelGGL(kern, dim3(blocks), dim3(512), 0, 0, d, (uint32_t)r);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms = 0; hipEventElapsedTime(&ms, e0, e1);
    ms /= 5;
    // per SIMD: 8 waves, each ITER * 8 * ni instructions
    const double cyc = ms * 1e-3 * 2.4e9 / (8.0 * ITER * 8.0 * ni);
    printf("%-34s %.3f ms  -> %.2f cycles per wave-instruction per SIMD, %.2f per three-input XOR\n", name, ms, cyc, cyc * ni);
    return ms;
}
int main() {
    uint32_t *d; hipMalloc(&d, 256 * 4 * 512 * 4);
    run("v_xor_b32 (one)", k_xor1, k_xor1_ni, d);
    run("v_xor_b32 x2 (hi ^ c ^ k)", k_xor2, k_xor2_ni, d);
    run("v_bitop3_b32 0x96 (hi ^ c ^ k)", k_bitop3, k_bitop3_ni, d);
    // a check of the truth table on the device: bitop3 0x96 is a ^ b ^ k
    uint32_t h[64];
    hipLaunchKernelGGL(k_bitop3, dim3(1), dim3(64), 0, 0, d, 3u);
    hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    uint32_t w[64];
    hipLaunchKernelGGL(k_xor2, dim3(1), dim3(64), 0, 0, d, 3u);
    hipMemcpy(w, d, sizeof(w), hipMemcpyDeviceToHost);
    int bad = 0;
    for (int i = 0; i < 64; ++i) bad += h[i] != w[i];
    printf("bitop3 0x96 against two XORs on 64 lanes: %s\n", bad ? "DIFFERENT" : "identical");
    hipFree(d);
    return bad != 0;
}
