// fk_split.h -- a rank's input split of a FASTA or FASTQ file (see fk_split.cpp).
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

namespace fk {

// One piece of a rank's input: literal bytes (a header prefix, the overlap, a final newline) or a
// byte range of the file.
struct SplitSeg {
    bool literal;
    std::string bytes;
    uint64_t off, len;  // file range (literal: off unused, len = bytes.size())
};

struct SplitPlan {
    std::vector<SplitSeg> segs;
    uint64_t total = 0;     // bytes the rank ingests
    uint64_t lo = 0, hi = 0;  // the rank's byte range of the file (its sequence starts at lo)
};

// The split of rank `rank` of `world` of the n-byte file open at fd for (k, sequence_type).
int plan_split(int fd, uint64_t n, int world, int rank, int k, int sequence_type, SplitPlan &plan, std::string &err);
// Bytes [pos, pos + len) of the rank's input into dst.
int read_split(int fd, uint64_t n, const SplitPlan &plan, uint64_t pos, uint64_t len, uint8_t *dst, std::string &err);

// ---- FASTQ (strict four-line records: "@name", sequence, "+[anything]", quality)
// A record starts at a line that begins with '@' and whose second-next line begins with '+' (exact
// for this grammar: a quality line beginning with '@' has a sequence line two lines after it).
//
// The last record start of bytes [lo, n) whose '@' line and '+' line both begin below n, or n when
// there is none.  lo must be a line start; at(p) returns byte p.  Scans backwards and stops at the
// first hit: a few lines unless a record is longer than that.  floor (>= lo): bytes below it are not
// looked at (at(floor - 1) aside), so a caller can bound the scan; a record start below it is not found.
template <class At>
uint64_t fastq_frontier_scan(At at, uint64_t lo, uint64_t n, uint64_t floor = 0) {
    constexpr uint64_t NONE = ~0ull;
    uint64_t l1 = NONE, l2 = NONE;  // the starts of the next line and of the one after it
    for (uint64_t p = n; p-- > (floor > lo ? floor : lo);) {
        if (p != lo && at(p - 1) != '\n') continue;
        if (l2 != NONE && at(p) == '@' && at(l2) == '+') return p;
        l2 = l1;
        l1 = p;
    }
    return n;
}

// The split of rank `rank` of `world` of an n-byte FASTQ file: the whole records whose '@' line
// starts in [rank * n / world, (rank + 1) * n / world); rank 0 also gets anything before the first
// record start, the last rank everything to the file's end.
int plan_split_fastq(int fd, uint64_t n, int world, int rank, SplitPlan &plan, std::string &err);

}  // namespace fk
