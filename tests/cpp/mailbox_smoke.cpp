// The two record formats of the mailbox (csrc/ssf_mailbox.hpp, the part that includes no HIP header) on the CPU: a record
// encoded word by word with SSF_ICP_REC_WORD is read back by icp_record_read, and every way a record can be incomplete is
// refused; the same for the integer records and int_record_read.  Built with -fsanitize=address,undefined by
// tests/test_mailbox.py.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../supersurfel_fusion_amd/csrc/ssf_mailbox.hpp"

typedef unsigned long long u64;

static int failures = 0;
#define EXPECT(cond)                                                                      \
    do {                                                                                  \
        if (!(cond)) { std::printf("%s: line %d: %s\n", what, __LINE__, #cond); failures++; } \
    } while (0)

// the record of sums[29] under seq, all 40 words through the macro
static void encode(const long long* sums, u64 seq, u64* rec40) {
    u64 pay[30];
    for (int p = 0; p < 29; p++) pay[p] = (u64)sums[p];
    pay[29] = ssf::icp_record_check(sums, seq);
    for (int w = 0; w < 40; w++) rec40[w] = SSF_ICP_REC_WORD(w, pay, seq);
}

// what icp_record_read takes for a pointer: the first `swap_at` loads come from a, the rest from b
struct Swapping {
    const u64 *a, *b;
    int swap_at;
    int* loads;                                  // (the reader takes its pointer by value)
    const volatile u64& operator[](int i) const { return ((*loads)++ < swap_at ? a : b)[i]; }
};

static void check_icp(const char* what, const long long* sums, u64 seq) {
    u64 rec[40];
    long long out[29];
    encode(sums, seq, rec);
    // the layout: five lines of seven payload words and the sequence number, the rest of line 5 zero
    for (int j = 0; j < 5; j++) EXPECT(rec[8 * j + 7] == seq);
    for (int p = 0; p < 29; p++) EXPECT(rec[SSF_ICP_REC_AT(p)] == (u64)sums[p]);
    EXPECT(rec[SSF_ICP_REC_AT(29)] == ssf::icp_record_check(sums, seq));
    for (int w = SSF_ICP_REC_AT(29) + 1; w < 39; w++) EXPECT(rec[w] == 0);
    for (int p = 0; p < 30; p++) {
        EXPECT(SSF_ICP_REC_AT(p) % 8 != 7 && SSF_ICP_REC_AT(p) < 40);
        if (p) EXPECT(SSF_ICP_REC_AT(p) > SSF_ICP_REC_AT(p - 1));
    }
    // read back
    std::memset(out, 0x5a, sizeof out);
    EXPECT(ssf::icp_record_read((const volatile u64*)rec, seq, out));
    for (int p = 0; p < 29; p++) EXPECT(out[p] == sums[p]);
    EXPECT(!ssf::icp_record_read((const volatile u64*)rec, seq + 1, out));
    // one line still carries the previous record's number
    for (int j = 0; j < 5; j++) {
        u64 r[40]; std::memcpy(r, rec, sizeof r);
        r[8 * j + 7] = seq - 1;
        EXPECT(!ssf::icp_record_read((const volatile u64*)r, seq, out));
    }
    // one payload word off by one; the check word off by one
    for (int p = 0; p < 30; p++) {
        u64 r[40]; std::memcpy(r, rec, sizeof r);
        r[SSF_ICP_REC_AT(p)] += 1;
        EXPECT(!ssf::icp_record_read((const volatile u64*)r, seq, out));
        r[SSF_ICP_REC_AT(p)] -= 2;
        EXPECT(!ssf::icp_record_read((const volatile u64*)r, seq, out));
    }
    // the next record (other sums, seq + 1) lands while this one is being read: after any number of loads short of all of
    // them -- 5 sequence words, 30 payload words, 5 sequence words again -- the read must be refused
    long long other[29];
    for (int p = 0; p < 29; p++) other[p] = (long long)((u64)sums[p] * 3u + (u64)p + 11u);
    u64 next[40];
    encode(other, seq + 1, next);
    for (int k = 0; k <= 40; k++) {
        int loads = 0;
        const bool ok = ssf::icp_record_read(Swapping{rec, next, k, &loads}, seq, out);
        EXPECT(ok == (k == 40));
        if (k == 40) EXPECT(loads == 40);
    }
    {   // ... in particular exactly between the reader's two looks at the sequence words, with the SAME sums under seq + 1
        u64 same_next[40];
        encode(sums, seq + 1, same_next);
        int loads = 0;
        EXPECT(!ssf::icp_record_read(Swapping{rec, same_next, 35, &loads}, seq, out));
        EXPECT(loads > 35);
    }
}

static void check_int(const char* what, int n, u64 seq) {
    std::vector<int> words(n), out(n, 0x5a5a5a5a);
    for (int i = 0; i < n; i++) words[i] = (i % 3 == 0) ? -1 /* 0xFFFFFFFF */ : (i % 3 == 1 ? (int)(0x80000000u + 12345u * i) : i * 7919);
    // the rule, restated: seq + the words as unsigned 32-bit values (a sign-extending sum would differ: there are -1 words)
    u64 want = seq, as_signed = seq;
    for (int i = 0; i < n; i++) { want += (u64)(unsigned int)words[i]; as_signed += (u64)(long long)words[i]; }
    EXPECT(want != as_signed);
    EXPECT(ssf::int_record_check(words.data(), n, seq) == want);
    volatile u64 check = want;
    EXPECT(ssf::int_record_read(words.data(), n, &check, seq, out.data()));
    for (int i = 0; i < n; i++) EXPECT(out[i] == words[i]);
    check = as_signed;
    EXPECT(!ssf::int_record_read(words.data(), n, &check, seq, out.data()));
    check = ssf::int_record_check(words.data(), n, seq + 1);              // a check word computed for another record number
    EXPECT(!ssf::int_record_read(words.data(), n, &check, seq, out.data()));
    check = want;
    EXPECT(!ssf::int_record_read(words.data(), n, &check, seq - 1, out.data()));
    for (int i = 0; i < n; i++) {                                          // one flipped bit in any word
        words[i] ^= 1 << (i % 32);
        EXPECT(!ssf::int_record_read(words.data(), n, &check, seq, out.data()));
        words[i] ^= 1 << (i % 32);
    }
    EXPECT(ssf::int_record_read(words.data(), n, &check, seq, out.data()));
}

int main() {
    long long full[29], neg[29], zero[29], mixed[29];
    for (int p = 0; p < 29; p++) {
        full[p] = (long long)(0xF123456789ABCDEFull * (u64)(2 * p + 1));       // all 64 bits in use, both signs
        neg[p] = -(long long)(1 + p) * 1000003ll;
        zero[p] = 0;
        mixed[p] = p % 3 == 0 ? 0 : (p % 3 == 1 ? -(1ll << (p + 20)) : (1ll << (p + 30)) + p);
    }
    full[0] = (long long)0x8000000000000000ull; full[1] = 0x7FFFFFFFFFFFFFFFll; full[2] = -1;
    const u64 seqs[3] = {1ull, 1ull << 32, ~0ull};
    for (int s = 0; s < 3; s++) {
        check_icp("icp record, 64-bit sums", full, seqs[s]);
        check_icp("icp record, negative sums", neg, seqs[s]);
        check_icp("icp record, zero", zero, seqs[s]);
        check_icp("icp record, mixed", mixed, seqs[s]);
        check_int("counter record", ssf::MAILBOX_COUNTER_WORDS, seqs[s]);
        check_int("shard-size record", ssf::MAILBOX_SHARD_WORDS, seqs[s]);
    }
    if (failures) { std::printf("mailbox_smoke: %d failures\n", failures); return 1; }
    std::printf("mailbox_smoke ok\n");
    return 0;
}
