// store_header_check.cpp -- a stand-alone program around the database header parser
// (fastkmer_amd/csrc/fk_db_header.h), built by tests/test_store.py with the host's address and
// undefined-behaviour sanitizers.  It takes a valid database file and a scratch directory, and feeds the
// parser every truncation of the file's header and every header byte changed in three ways (inverted,
// 0x00, 0xff), in memory and through files.  Every answer must be FK_OK, FK_E_INVALID or FK_E_IO, and
// the untouched file must parse.  Exit status 0 and one summary line when all of that held.
#include <stdio.h>

#include <string>
#include <vector>

#include "../fastkmer_amd/csrc/fk_db_header.h"

using namespace fk;

static bool known(int rc) { return rc == FK_OK || rc == FK_E_INVALID || rc == FK_E_IO; }

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s database scratch_dir\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> file;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint8_t buf[1 << 16];
    for (size_t got; (got = fread(buf, 1, sizeof(buf), in)) > 0;) file.insert(file.end(), buf, buf + got);
    fclose(in);
    fk_db_info h;
    std::vector<DbBin> bins;
    std::string err;
    if (db_read_header(argv[1], &h, &bins, &err) != FK_OK) {
        fprintf(stderr, "the untouched file is refused: %s\n", err.c_str());
        return 1;
    }
    const size_t hb = (size_t)(DB_FIXED + DB_BIN_ENTRY * bins.size());
    size_t tried = 0, refused = 0;
    // in memory: every truncation of the header, the file's size kept and cut with it
    for (size_t have = 0; have <= hb; ++have) {
        std::vector<uint8_t> part(file.begin(), file.begin() + have);  // its own allocation: a read past it is caught
        for (uint64_t size : {(uint64_t)file.size(), (uint64_t)have}) {
            const int rc = db_parse_header(part.data(), have, size, &h, &bins, &err);
            if (!known(rc) || (have < hb && rc == FK_OK)) {
                fprintf(stderr, "%zu header bytes of a %llu-byte file: code %d\n", have, (unsigned long long)size, rc);
                return 1;
            }
            ++tried, refused += rc != FK_OK;
        }
    }
    // in memory: every header byte changed
    for (size_t i = 0; i < hb; ++i) {
        for (int how = 0; how < 3; ++how) {
            std::vector<uint8_t> part(file.begin(), file.begin() + hb);
            part[i] = how == 0 ? (uint8_t)~part[i] : how == 1 ? 0x00 : 0xff;
            const int rc = db_parse_header(part.data(), hb, file.size(), &h, &bins, &err);
            if (!known(rc)) {
                fprintf(stderr, "byte %zu changed: code %d\n", i, rc);
                return 1;
            }
            ++tried, refused += rc != FK_OK;
        }
    }
    // through files: truncations at every 4 bytes of the header and around the sections' end, and the 16
    // bytes that size the header changed (a header that claims more bins than the file holds)
    const std::string path = std::string(argv[2]) + "/mutant.fkdb";
    auto run_file = [&](const std::vector<uint8_t> &bytes) {
        FILE *out = fopen(path.c_str(), "wb");
        if (!out || (bytes.size() && fwrite(bytes.data(), 1, bytes.size(), out) != bytes.size())) return -100;
        fclose(out);
        return db_read_header(path.c_str(), &h, &bins, &err);
    };
    std::vector<size_t> cuts;
    for (size_t n = 0; n <= hb + 8; n += 4) cuts.push_back(n);
    cuts.push_back(file.size() - 1);
    for (size_t n : cuts) {
        const int rc = run_file(std::vector<uint8_t>(file.begin(), file.begin() + n));
        if (rc != FK_E_IO) {
            fprintf(stderr, "a file cut to %zu bytes: code %d, want FK_E_IO (%s)\n", n, rc, err.c_str());
            return 1;
        }
        ++tried, ++refused;
    }
    for (size_t i = 0; i < 48; ++i) {
        for (int how = 0; how < 3; ++how) {
            std::vector<uint8_t> bytes = file;
            bytes[i] = how == 0 ? (uint8_t)~bytes[i] : how == 1 ? 0x00 : 0xff;
            const int rc = run_file(bytes);
            if (!known(rc)) {
                fprintf(stderr, "file byte %zu changed: code %d\n", i, rc);
                return 1;
            }
            ++tried, refused += rc != FK_OK;
        }
    }
    std::vector<uint8_t> longer = file;
    longer.push_back(0);
    if (run_file(longer) != FK_E_IO || err.find("trailing bytes") == std::string::npos) {
        fprintf(stderr, "a file one byte longer: %s\n", err.c_str());
        return 1;
    }
    remove(path.c_str());
    printf("store_header_check: %zu headers parsed, %zu refused, no sanitizer report\n", tried + 1, refused + 1);
    return 0;
}
