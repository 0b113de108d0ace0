// ssf_mailbox.hpp -- the two self-validating record formats of the host-mapped mailbox (Mailbox, ssf_device.hpp) and of the
// peer-to-peer exchange regions: where the words sit, the check words, one attempt of the host's read and, behind __HIPCC__,
// the device's writers.  The first part includes no HIP header: tests/cpp/mailbox_smoke.cpp runs it on the CPU.  (Its
// functions are static: a copy the compiler does not inline must not become a symbol of the library.)
#pragma once

namespace ssf {

// ---- the ICP record: 29 sums + a check word, as five 64-byte lines of 7 payload words + the sequence number ---------------
// One wave store writes all 40 words; a reader accepts the record when every line carries the awaited sequence number and
// the check word matches -- no ordering between the stores, no wait for write acknowledgements in between.
// word w of the record for payload p[0..29] and sequence number seq (the unused words of line 5: 0) ...
#define SSF_ICP_REC_WORD(w, p, seq) ((((w) & 7) == 7) ? (unsigned long long)(seq) : ((7 * ((w) >> 3) + ((w) & 7)) < 30 ? (unsigned long long)(p)[7 * ((w) >> 3) + ((w) & 7)] : 0ull))
// ... and the inverse: payload word p sits at word
#define SSF_ICP_REC_AT(p) (8 * ((p) / 7) + (p) % 7)
// the check word: seq + the 29 sums
static inline unsigned long long icp_record_check(const long long* sums29, unsigned long long seq) {
    unsigned long long c = seq;
    for (int p = 0; p < 29; p++) c += (unsigned long long)sums29[p];
    return c;
}
// ONE attempt of the host's read: all five lines carry seq, the sums are copied (out29 is written whatever the outcome), the
// check word matches and the lines still carry seq.  false = a record in flight.  (Rec: const volatile unsigned long long*;
// a template so that the CPU test can change the record between two loads.)
template <typename Rec>
static inline bool icp_record_read(Rec rec, unsigned long long seq, long long out29[29]) {
    for (int j = 0; j < 5; j++)
        if (__atomic_load_n(&rec[8 * j + 7], __ATOMIC_ACQUIRE) != seq) return false;
    for (int p = 0; p < 29; p++) out29[p] = (long long)__atomic_load_n(&rec[SSF_ICP_REC_AT(p)], __ATOMIC_RELAXED);
    const unsigned long long w29 = __atomic_load_n(&rec[SSF_ICP_REC_AT(29)], __ATOMIC_RELAXED);
    for (int j = 0; j < 5; j++)
        if (__atomic_load_n(&rec[8 * j + 7], __ATOMIC_ACQUIRE) != seq) return false;
    return icp_record_check(out29, seq) == w29;
}

// ---- the integer record: n words, the check word and, once those stores are acknowledged, the sequence word ---------------
// (Mailbox::cnt, the frame's Counters: sizeof(Counters) / 4 words, asserted in ssf_device.hpp; Mailbox::all_cnt, Counters::last
// of every rank)
#define SSF_MAX_RANKS 64
enum { MAILBOX_COUNTER_WORDS = 24, MAILBOX_SHARD_WORDS = 5 * SSF_MAX_RANKS };
// the check word: seq + the words as UNSIGNED 32-bit values
static inline unsigned long long int_record_check(const int* words, int n, unsigned long long seq) {
    unsigned long long c = seq;
    for (int i = 0; i < n; i++) c += (unsigned long long)(unsigned int)words[i];
    return c;
}
// ONE attempt of the host's read, behind the sequence word's arrival (out is written whatever the outcome); false = torn
static inline bool int_record_read(const int* words, int n, const volatile unsigned long long* check, unsigned long long seq, int* out) {
    for (int i = 0; i < n; i++) out[i] = __atomic_load_n(&words[i], __ATOMIC_RELAXED);
    return int_record_check(out, n, seq) == __atomic_load_n(check, __ATOMIC_ACQUIRE);
}

#ifdef __HIPCC__
// ---- the device's side: system-scope stores (the destination is host memory or a peer's exchange region) ------------------
__device__ __forceinline__ long long wsum64(long long v) {       // the sum over a wave's 64 lanes, told to every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Wave 0 of a workgroup, all 64 lanes, l = the lane: tot = sum l in lanes 0..28 and 0 in the others, pay = 30 words of LDS.
// LDS operations of one wave execute in order, so behind lgkmcnt(0) every lane reads what the others wrote (no barrier),
// and 40 lanes store the five lines in one instruction.
__device__ __forceinline__ void icp_record_store(unsigned long long* dst, long long tot, unsigned long long seq, unsigned long long* pay, unsigned int l) {
    if (l < 29) pay[l] = (unsigned long long)tot;
    const unsigned long long check = (unsigned long long)wsum64(tot) + seq;
    if (l == 0) pay[29] = check;
    __builtin_amdgcn_s_waitcnt(0xc07f);       // lgkmcnt(0)
    if (l < 40) __hip_atomic_store(&dst[l], SSF_ICP_REC_WORD(l, pay, seq), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// the integer record by ONE thread (src: values in registers) ...
__device__ __forceinline__ void int_record_store(int* dst_words, const int* src, int n, unsigned long long* check_word, unsigned long long* seq_word,
                                                 unsigned long long seq) {
    unsigned long long check = seq;
    for (int i = 0; i < n; i++) {
        __hip_atomic_store(&dst_words[i], src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        check += (unsigned long long)(unsigned int)src[i];
    }
    __hip_atomic_store(check_word, check, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // payload write-through stores acknowledged
    __hip_atomic_store(seq_word, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// ... by one wave, the end of a record whose words the lanes have stored themselves (part: the sum of this lane's words as
// unsigned 32-bit values; first: lane 0) ...
__device__ __forceinline__ void int_record_close(unsigned long long part, unsigned long long* check_word, unsigned long long* seq_word,
                                                 unsigned long long seq, bool first) {
    const unsigned long long check = (unsigned long long)wsum64((long long)part) + seq;
    if (first) __hip_atomic_store(check_word, check, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (first) __hip_atomic_store(seq_word, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// ... and the whole record by one wave, lane-strided over src in device memory
__device__ __forceinline__ void int_record_store(int* dst_words, const int* __restrict__ src, int n, unsigned long long* check_word,
                                                 unsigned long long* seq_word, unsigned long long seq, int l) {
    unsigned long long part = 0;
    for (int i = l; i < n; i += 64) {
        const int v = src[i];
        __hip_atomic_store(&dst_words[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        part += (unsigned long long)(unsigned int)v;
    }
    int_record_close(part, check_word, seq_word, seq, l == 0);
}
#endif

}  // namespace ssf
