// fk_db_header.h -- the database file's header (include/fastkmer.h, "export, import and the database
// file"): its layout, its writer and the only parser of a file's bytes.  Host only and free of HIP, so
// that it compiles into a stand-alone program under the host sanitizers (tests/store_header_check.cpp).
#pragma once

#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/fastkmer.h"

namespace fk {

constexpr char DB_MAGIC[8] = {'F', 'K', 'M', 'E', 'R', 'D', 'B', '\0'};
constexpr uint32_t DB_VERSION = 1;
constexpr uint64_t DB_FIXED = 72;        // bytes before the bin table
constexpr uint64_t DB_BIN_ENTRY = 16;    // {u32 bin, u32 0, u64 distinct}
constexpr int32_t DB_MAX_BINS = 1 << 22; // fk_config_validate: a record header holds 22 bits of bin

struct DbBin {
    uint32_t bin;
    uint64_t distinct;
};

// little-endian fields, whatever the host's alignment rules
inline uint32_t db_get32(const uint8_t *p) {
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
inline uint64_t db_get64(const uint8_t *p) { return (uint64_t)db_get32(p) | (uint64_t)db_get32(p + 4) << 32; }
inline void db_put32(uint8_t *p, uint32_t v) {
    for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
inline void db_put64(uint8_t *p, uint64_t v) {
    for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
}

// The header bytes a file declares: p holds its first `have` >= 16 bytes.  0 when they are no header
// (db_parse_header names the reason).
inline uint64_t db_header_bytes(const uint8_t *p, size_t have) {
    if (have < 16 || memcmp(p, DB_MAGIC, 8) != 0 || db_get32(p + 8) != DB_VERSION) return 0;
    const uint64_t hb = db_get32(p + 12);
    if (hb < DB_FIXED || hb % 8 || (hb - DB_FIXED) % DB_BIN_ENTRY || (hb - DB_FIXED) / DB_BIN_ENTRY > (uint64_t)DB_MAX_BINS)
        return 0;
    return hb;
}

// Parses and validates a header: p holds the file's first `have` bytes (as many of its header bytes as
// the file has), file_bytes the file's size.  FK_OK, or FK_E_INVALID / FK_E_IO with the reason in *err.
// bins (may be null) receives the bin table.
inline int db_parse_header(const uint8_t *p, size_t have, uint64_t file_bytes, fk_db_info *out, std::vector<DbBin> *bins,
                           std::string *err) {
    auto fail = [&](int code, const std::string &why) {
        *err = why;
        return code;
    };
    memset(out, 0, sizeof(*out));
    out->file_bytes = file_bytes;
    if (have < 8) return fail(FK_E_IO, "truncated: the file ends inside the magic");
    if (memcmp(p, DB_MAGIC, 8) != 0) return fail(FK_E_INVALID, "not a k-mer database: wrong magic");
    if (have < 16) return fail(FK_E_IO, "truncated: the file ends inside the header");
    const uint32_t version = db_get32(p + 8);
    if (version != DB_VERSION)
        return fail(FK_E_INVALID, "database version " + std::to_string(version) + ", this library reads version 1");
    out->version = (int32_t)version;
    const uint64_t hb = db_get32(p + 12);
    if (hb < DB_FIXED || hb % 8)
        return fail(FK_E_INVALID, "header bytes " + std::to_string(hb) + ": not a multiple of 8 of at least 72");
    if (have < DB_FIXED) return fail(FK_E_IO, "truncated: the file ends inside the header");
    out->k = (int32_t)db_get32(p + 16);
    out->m = (int32_t)db_get32(p + 20);
    out->bins = (int32_t)db_get32(p + 24);
    out->key_words = (int32_t)db_get32(p + 28);
    out->n_ranks = (int32_t)db_get32(p + 32);
    out->rank = (int32_t)db_get32(p + 36);
    const uint32_t stored = db_get32(p + 40);
    out->distinct = db_get64(p + 48);
    out->kmers = db_get64(p + 56);
    out->checksum = db_get64(p + 64);
    if (out->k < 1 || out->k > 64) return fail(FK_E_INVALID, "k = " + std::to_string(out->k) + " outside 1 .. 64");
    if (out->m < 1 || out->m > 15 || out->m > out->k)
        return fail(FK_E_INVALID, "m = " + std::to_string(out->m) + " outside 1 .. min(15, k)");
    if (out->bins < 1 || out->bins > DB_MAX_BINS || (uint64_t)out->bins > (1ull << (2 * out->m)))
        return fail(FK_E_INVALID, "bins = " + std::to_string(out->bins) + " outside 1 .. min(4^m, 2^22)");
    if (out->key_words != (out->k > 32 ? 2 : 1))
        return fail(FK_E_INVALID, "key_words = " + std::to_string(out->key_words) + " contradicts k = " + std::to_string(out->k));
    if (out->n_ranks < 1 || out->rank < 0 || out->rank >= out->n_ranks)
        return fail(FK_E_INVALID, "rank " + std::to_string(out->rank) + " of " + std::to_string(out->n_ranks));
    if (stored > (uint32_t)out->bins)
        return fail(FK_E_INVALID, "stored_bins = " + std::to_string(stored) + " above bins = " + std::to_string(out->bins));
    out->stored_bins = (int32_t)stored;
    if (hb != DB_FIXED + DB_BIN_ENTRY * stored)
        return fail(FK_E_INVALID, "header bytes " + std::to_string(hb) + " do not hold " + std::to_string(stored) + " stored bins");
    if (db_get32(p + 44) != 0) return fail(FK_E_INVALID, "the reserved word at offset 44 is not 0");
    if (have < hb) return fail(FK_E_IO, "truncated: the file ends inside the bin table");
    if (bins) bins->clear();
    uint64_t sum = 0;
    int64_t last = -1;
    for (uint32_t i = 0; i < stored; ++i) {
        const uint8_t *e = p + DB_FIXED + DB_BIN_ENTRY * i;
        const uint32_t b = db_get32(e);
        const uint64_t d = db_get64(e + 8);
        if (b >= (uint32_t)out->bins)
            return fail(FK_E_INVALID, "stored bin " + std::to_string(b) + " is not below bins = " + std::to_string(out->bins));
        if ((int64_t)b <= last) return fail(FK_E_INVALID, "the stored bins do not ascend at entry " + std::to_string(i));
        if (db_get32(e + 4) != 0) return fail(FK_E_INVALID, "the reserved word of bin entry " + std::to_string(i) + " is not 0");
        if (d == 0) return fail(FK_E_INVALID, "stored bin " + std::to_string(b) + " is empty");
        if (d > UINT64_MAX - sum) return fail(FK_E_INVALID, "the bins' sizes overflow");
        sum += d;
        last = b;
        if (bins) bins->push_back(DbBin{b, d});
    }
    if (sum != out->distinct)
        return fail(FK_E_INVALID, "the bins' sizes sum to " + std::to_string(sum) + ", distinct = " + std::to_string(out->distinct));
    if (out->kmers < out->distinct) return fail(FK_E_INVALID, "kmers below distinct: a count would be 0");
    const uint64_t per = (uint64_t)out->key_words * 8 + 4;
    if (out->distinct > (UINT64_MAX - hb) / per) return fail(FK_E_INVALID, "distinct overflows the file's size");
    const uint64_t want = hb + out->distinct * per;
    if (file_bytes < want)
        return fail(FK_E_IO, "truncated: " + std::to_string(file_bytes) + " bytes, the header says " + std::to_string(want));
    if (file_bytes > want)
        return fail(FK_E_IO, "trailing bytes: " + std::to_string(file_bytes) + " bytes, the header says " + std::to_string(want));
    return FK_OK;
}

// The header of a file to write; bins: the non-empty bins ascending.
inline std::vector<uint8_t> db_build_header(const fk_db_info &h, const std::vector<DbBin> &bins) {
    std::vector<uint8_t> b(DB_FIXED + DB_BIN_ENTRY * bins.size(), 0);
    memcpy(b.data(), DB_MAGIC, 8);
    db_put32(&b[8], DB_VERSION);
    db_put32(&b[12], (uint32_t)b.size());
    const int32_t f[6] = {h.k, h.m, h.bins, h.key_words, h.n_ranks, h.rank};
    for (int i = 0; i < 6; ++i) db_put32(&b[16 + 4 * i], (uint32_t)f[i]);
    db_put32(&b[40], (uint32_t)bins.size());
    db_put64(&b[48], h.distinct);
    db_put64(&b[56], h.kmers);
    db_put64(&b[64], h.checksum);
    for (size_t i = 0; i < bins.size(); ++i) {
        db_put32(&b[DB_FIXED + DB_BIN_ENTRY * i], bins[i].bin);
        db_put64(&b[DB_FIXED + DB_BIN_ENTRY * i + 8], bins[i].distinct);
    }
    return b;
}

// fk_db_info_read without the thread's error message: the file at `path` opened, sized and parsed.
inline int db_read_header(const char *path, fk_db_info *out, std::vector<DbBin> *bins, std::string *err) {
    memset(out, 0, sizeof(*out));
    const int fd = open(path, O_RDONLY);
    if (fd < 0) {
        *err = std::string("cannot open ") + path + ": " + strerror(errno);
        return FK_E_IO;
    }
    struct stat sb;
    if (fstat(fd, &sb) != 0) {
        *err = std::string("cannot stat ") + path + ": " + strerror(errno);
        close(fd);
        return FK_E_IO;
    }
    const uint64_t size = (uint64_t)sb.st_size;
    // the fixed part says how long the header is; a file that is no database is parsed from it alone
    std::vector<uint8_t> buf(DB_FIXED);
    auto fill = [&](size_t from, size_t to) {  // bytes [from, to) of the file, as far as it reaches
        while (from < to) {
            const ssize_t got = pread(fd, buf.data() + from, to - from, (off_t)from);
            if (got < 0 && errno == EINTR) continue;
            if (got <= 0) break;
            from += (size_t)got;
        }
        return from;
    };
    size_t have = fill(0, (size_t)std::min<uint64_t>(DB_FIXED, size));
    const uint64_t hb = db_header_bytes(buf.data(), have);
    if (hb > DB_FIXED && have == DB_FIXED) {
        const size_t want = (size_t)std::min<uint64_t>(hb, size);
        buf.resize(want);
        have = fill(DB_FIXED, want);
    }
    close(fd);
    const int rc = db_parse_header(buf.data(), have, size, out, bins, err);
    if (rc != FK_OK) *err = std::string(path) + ": " + *err;
    return rc;
}

}  // namespace fk
