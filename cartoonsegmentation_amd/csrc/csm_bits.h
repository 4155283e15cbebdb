// csm_bits.h -- device pieces the codecs share: the workgroup reductions and scans over LDS, the LSB-first bit writer, and the
// scanner that splits a row into runs of equal elements.  Header-only; include it from a .hip file.
//
// Every helper that takes `sh` is called by ALL kBlock threads of a one-dimensional workgroup of exactly kBlock threads (a
// compile-time constant, so the loops unroll), with kBlock elements of LDS that it may overwrite.  Each begins with a barrier
// behind its first LDS store and ends with one behind its last LDS read: LDS the caller wrote before the call is visible to every
// thread after it, and `sh` may be reused at once.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace csm_bits {

// sum of v over the workgroup, in every thread
template <int kBlock, typename T> __device__ T block_sum(T v, T *sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = kBlock >> 1; d > 0; d >>= 1) {
        if (t < d) sh[t] += sh[t + d];
        __syncthreads();
    }
    const T r = sh[0];
    __syncthreads();
    return r;
}

// exclusive prefix of v over the workgroup, and the total
template <int kBlock, typename T> __device__ T block_exclusive(T v, T *sh, T &total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
        const T w = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += w;
        __syncthreads();
    }
    total = sh[kBlock - 1];
    const T ex = t ? sh[t - 1] : 0;
    __syncthreads();
    return ex;
}

// minimum of v over the threads AFTER this one (`none` for the last)
template <int kBlock, typename T> __device__ T block_min_after(T v, T none, T *sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < kBlock; d <<= 1) {
        const T w = t + d < kBlock ? sh[t + d] : none;
        __syncthreads();
        sh[t] = min(sh[t], w);
        __syncthreads();
    }
    const T r = t + 1 < kBlock ? sh[t + 1] : none;
    __syncthreads();
    return r;
}

// LSB-first bit writer into a buffer of 32-bit words that was ZEROED before the kernel ran.  A thread ORs each word it completes
// once; the words at its two ends are shared with its neighbours.  A completed word that is zero is not written: the buffer
// already holds it, so the bytes are those of a writer that ORs every word.  Nothing is written at or past word `limit`.
struct BitSink {
    uint32_t *buf;
    int64_t w, limit;
    unsigned long long acc;
    int fill;
    __device__ __forceinline__ void open(uint32_t *b, int64_t pos, int64_t lim) { buf = b; w = pos >> 5; fill = (int)(pos & 31); acc = 0; limit = lim; }
    // the n low bits of v, 0 <= n <= 32
    __device__ __forceinline__ void put(uint32_t v, int n) {
        acc |= (unsigned long long)v << fill;
        fill += n;
        if (fill >= 32) {
            if (w < limit && (uint32_t)acc) atomicOr(buf + w, (uint32_t)acc);
            ++w;
            acc >>= 32;
            fill -= 32;
        }
    }
    __device__ __forceinline__ void close() { if (fill && w < limit && (uint32_t)acc) atomicOr(buf + w, (uint32_t)acc); fill = 0; acc = 0; }
};

// ---- runs of equal elements ---------------------------------------------------------------------------------------------------
// A row F[0, L) split among the threads: thread t takes the stretch [i0, i1) of consecutive elements and the runs that START
// there.  first = the first run start of the stretch (i1 if none), next = the first run start at or after i1 (L if none).
struct RunStretch {
    int i0, i1, first, next;
};

// all threads; sh: kBlock ints of LDS (block_min_after's barriers apply)
template <int kBlock, typename E> __device__ __forceinline__ RunStretch run_stretch(const E *__restrict__ F, int L, int *sh) {
    const int t = threadIdx.x;
    const int per = (L + kBlock - 1) / kBlock;
    RunStretch s;
    s.i0 = min(L, t * per); s.i1 = min(L, s.i0 + per);
    s.first = L;
    for (int i = s.i0; i < s.i1; ++i) {
        if (i == 0 || F[i] != F[i - 1]) { s.first = i; break; }
    }
    s.next = block_min_after<kBlock>(s.first, L, sh);
    if (s.first >= s.i1) s.first = s.i1;
    return s;
}

// hands every run that starts in the stretch to sink.run(value, length)
template <typename E, typename Sink> __device__ __forceinline__ void parse_chunk(const E *__restrict__ F, const RunStretch &s, Sink &sink) {
    int b = s.first;
    while (b < s.i1) {
        const E v = F[b];
        int e = b + 1;
        while (e < s.i1 && F[e] == v) ++e;
        if (e == s.i1) e = s.next;                          // the run goes on to the next start (which may be i1 itself)
        sink.run(v, e - b);
        b = e;
    }
}

}  // namespace csm_bits
