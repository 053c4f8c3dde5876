// fk_cli.cpp -- command-line driver with the reference's positional arguments.
//
//   fastkmer-cli [LocalTestKmerCounter|TestKmerCounter] k m x B useHT sequenceType
//                inputPath outputPath prefix write enableKryo useCustomPartitioner [numPartitionTasks]
//
// Argument order and meaning follow skc.test.LocalTestKmerCounter.main
// (LocalTestKmerCounter.scala:35-48) and TestKmerCounter.main
// (TestKmerCounter.scala:34-47); the output directory is
// TestConfiguration.outputDir (test/package.scala:33).  enableKryo selects a
// JVM serializer and useCustomPartitioner a Spark placement: neither changes
// the counts, both are accepted and reported.
//
// Beyond the reference (read here only, the positional contract is untouched; with none of them
// set the output is byte-identical):
//   FASTKMER_CLI_MIN_COUNT / FASTKMER_CLI_MAX_COUNT  with write = 1 the bin files hold only the
//       k-mers with min <= count <= max (fk_write_bins_range; defaults 1 / no upper bound)
//   FASTKMER_CLI_SPECTRUM=<n>  writes <outputDir>/spectrum.txt, "<c>\t<distinct k-mers>\n" for the
//       nonzero entries of the n-entry abundance spectrum, ascending; the last entry (count >= n - 1)
//       as ">=<n - 1>\t..."; written whether or not write is set
//   FASTKMER_CLI_FORMAT=fasta|fastq|auto  the input's format (default fasta; auto: FASTQ iff the
//       file's first byte is '@'); any other value is a usage error
//   FASTKMER_CLI_MIN_QUAL=<q> / FASTKMER_CLI_QUAL_OFFSET=33|64  FASTQ only: bases with a Phred score
//       below q count as N (default 0: qualities ignored) / the quality encoding (default 33)
//   FASTKMER_CLI_READS=<file>  after the count, the reads of <file> (the job's input format and quality
//       settings) are profiled against the result: <outputDir>/read_stats.tsv, one line per read,
//       "index\tlength\twindows\thits\tmin\tmedian\tmax\tsum" (fk_read_stats; hits counts the k-mers with
//       FASTKMER_CLI_MIN_COUNT <= count <= FASTKMER_CLI_MAX_COUNT); needs useHT = 0, else a usage error
//   FASTKMER_CLI_COMPARE=<file>  after the count, <file> is counted in a second context of the same
//       configuration, input format and quality settings and the two results are compared:
//       <outputDir>/compare.tsv, "<count in the input>\t<count in file>\t<distinct k-mers>\n" for the nonzero
//       entries of the joint count matrix (fk_compare), row-major; needs useHT = 0, else a usage error
//       a <file> that begins with the database magic "FKMERDB\0" (FASTKMER_CLI_SAVE, fk_save) is loaded
//       (fk_load) instead of counted
//   FASTKMER_CLI_SAVE=<file>  after the count, the result is saved as a database file (fk_save); needs
//       useHT = 0, else a usage error
//   FASTKMER_CLI_COMPARE_N=<n>  rows = cols = n of that matrix, 2 .. 4096 (default 256): the last row and
//       column collect the counts >= n - 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "../../include/fastkmer.h"

static int usage(const char *argv0) {
    fprintf(stderr,
            "usage: %s [LocalTestKmerCounter|TestKmerCounter] k m x B useHT sequenceType inputPath outputPath "
            "prefix write enableKryo useCustomPartitioner [numPartitionTasks]\n",
            argv0);
    return 2;
}

static bool parse_int(const char *s, int *out) {
    char *end = nullptr;
    long v = strtol(s, &end, 10);
    if (!s[0] || *end) return false;
    *out = (int)v;
    return true;
}

// an optional unsigned environment value in [lo, hi]; false (with a message) when set and malformed
static bool env_u64(const char *name, uint64_t lo, uint64_t hi, bool *set, uint64_t *out) {
    const char *v = getenv(name);
    *set = v && v[0];
    if (!*set) return true;
    char *end = nullptr;
    const unsigned long long x = strtoull(v, &end, 10);
    if (*end || v[0] == '-' || x < lo || x > hi) {
        fprintf(stderr, "invalid configuration: %s=%s is not an integer in [%llu, %llu]\n", name, v,
                (unsigned long long)lo, (unsigned long long)hi);
        return false;
    }
    *out = x;
    return true;
}

int main(int argc, char **argv) {
    int a = 1;
    std::string driver = "LocalTestKmerCounter";
    if (argc > 1 && (!strcmp(argv[1], "LocalTestKmerCounter") || !strcmp(argv[1], "TestKmerCounter") ||
                     !strcmp(argv[1], "skc.test.LocalTestKmerCounter") || !strcmp(argv[1], "skc.test.TestKmerCounter"))) {
        driver = argv[1];
        a = 2;
    }
    if (argc - a < 12) return usage(argv[0]);
    fk_config cfg;
    fk_config_init(&cfg);
    int use_ht, write, kryo, part, ntasks = 0;
    if (!parse_int(argv[a + 0], &cfg.k) || !parse_int(argv[a + 1], &cfg.m) || !parse_int(argv[a + 2], &cfg.x) ||
        !parse_int(argv[a + 3], &cfg.B) || !parse_int(argv[a + 4], &use_ht) ||
        !parse_int(argv[a + 5], &cfg.sequence_type) || !parse_int(argv[a + 9], &write) ||
        !parse_int(argv[a + 10], &kryo) || !parse_int(argv[a + 11], &part))
        return usage(argv[0]);
    cfg.use_ht = use_ht == 1 ? 1 : 0;  // args(4).toInt == 1
    cfg.write = write == 1 ? 1 : 0;
    if (part == 1) {
        if (argc - a < 13 || !parse_int(argv[a + 12], &ntasks)) return usage(argv[0]);
    }
    const char *input = argv[a + 6];
    const char *output = argv[a + 7];
    const char *prefix = argv[a + 8];
    if (fk_config_validate(&cfg) != FK_OK) {
        fprintf(stderr, "invalid configuration: %s\n", fk_last_error());
        return 1;
    }
    bool has_min, has_max, has_spec;
    uint64_t min_count = 1, max_count = UINT32_MAX, spec_n = 0;
    if (!env_u64("FASTKMER_CLI_MIN_COUNT", 1, UINT32_MAX, &has_min, &min_count) ||
        !env_u64("FASTKMER_CLI_MAX_COUNT", 1, UINT32_MAX, &has_max, &max_count) ||
        !env_u64("FASTKMER_CLI_SPECTRUM", 2, 1ull << 28, &has_spec, &spec_n))
        return 1;
    if (min_count > max_count) {
        fprintf(stderr, "invalid configuration: FASTKMER_CLI_MIN_COUNT > FASTKMER_CLI_MAX_COUNT\n");
        return 1;
    }
    const bool ranged = has_min || has_max;
    const char *fmt_env = getenv("FASTKMER_CLI_FORMAT");
    int format = FK_FORMAT_FASTA;  // -1: auto
    if (fmt_env && fmt_env[0]) {
        if (!strcmp(fmt_env, "fastq"))
            format = FK_FORMAT_FASTQ;
        else if (!strcmp(fmt_env, "auto"))
            format = -1;
        else if (strcmp(fmt_env, "fasta")) {
            fprintf(stderr, "FASTKMER_CLI_FORMAT=%s: expected fasta, fastq or auto\n", fmt_env);
            return usage(argv[0]);
        }
    }
    bool has_minq, has_qoff;
    uint64_t min_qual = 0, qual_off = 33;
    if (!env_u64("FASTKMER_CLI_MIN_QUAL", 0, 93, &has_minq, &min_qual) ||
        !env_u64("FASTKMER_CLI_QUAL_OFFSET", 33, 64, &has_qoff, &qual_off))
        return 1;
    const char *reads_path = getenv("FASTKMER_CLI_READS");
    if (reads_path && !reads_path[0]) reads_path = nullptr;
    if (reads_path && cfg.use_ht) {
        fprintf(stderr, "FASTKMER_CLI_READS needs the sorted count (useHT = 0): a useHT = 1 result cannot be looked up\n");
        return usage(argv[0]);
    }
    const char *compare_path = getenv("FASTKMER_CLI_COMPARE");
    if (compare_path && !compare_path[0]) compare_path = nullptr;
    bool has_cmp_n;
    uint64_t cmp_n = 256;
    if (!env_u64("FASTKMER_CLI_COMPARE_N", 2, 4096, &has_cmp_n, &cmp_n)) return usage(argv[0]);
    if (compare_path && cfg.use_ht) {
        fprintf(stderr, "FASTKMER_CLI_COMPARE needs the sorted count (useHT = 0): a useHT = 1 result cannot be looked up\n");
        return usage(argv[0]);
    }
    const char *save_path = getenv("FASTKMER_CLI_SAVE");
    if (save_path && !save_path[0]) save_path = nullptr;
    if (save_path && cfg.use_ht) {
        fprintf(stderr, "FASTKMER_CLI_SAVE needs the sorted count (useHT = 0): a useHT = 1 result cannot be looked up\n");
        return usage(argv[0]);
    }
    char outdir[4096];
    fk_output_dir(&cfg, output, prefix, outdir, sizeof(outdir));
    // TestConfiguration.toString (test/package.scala:37-39)
    printf("Kmer counting on MI355X (%s). \nTest parameters:\nDataset: %s\nk: %d\nm: %d\nx: %d\nb: %d\n"
           "Sequence type: %d\nUsing HT:  %s\nWriting: %s\nUsing Kryo Serializer: %s\n"
           "Multiprocessor Scheduliong Partitioning: %s",
           driver.c_str(), input, cfg.k, cfg.m, cfg.x, fk_clamped_bins(cfg.m, cfg.B), cfg.sequence_type,
           cfg.use_ht ? "true" : "false", cfg.write ? "true" : "false", kryo == 1 ? "true (no effect)" : "false",
           part == 1 ? "true (no effect on one GPU)" : "false");
    if (part == 1) printf("\t no. partition tasks: %d", ntasks);
    printf("\n");

    // the input is memory-mapped and streamed to the device in windows (FASTdoop reads its
    // splits the same way, SBKC:1009-1012): fk_ingest appends each window and the fused map
    // runs over the tiles that have landed while the next window is in flight
    const int fd = open(input, O_RDONLY);
    if (fd < 0) {
        fprintf(stderr, "cannot open %s\n", input);
        return 1;
    }
    struct stat sb;
    if (fstat(fd, &sb) != 0) {
        fprintf(stderr, "cannot stat %s\n", input);
        close(fd);
        return 1;
    }
    const size_t size = (size_t)sb.st_size;
    const uint8_t *map = nullptr;
    if (size) {
        void *p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (p == MAP_FAILED) {
            fprintf(stderr, "cannot map %s\n", input);
            close(fd);
            return 1;
        }
        (void)madvise(p, size, MADV_SEQUENTIAL);
        map = (const uint8_t *)p;
    }
    fk_ctx *ctx = nullptr;
    if (fk_create(&cfg, &ctx) != FK_OK) {
        fprintf(stderr, "fk_create: %s\n", fk_last_error());
        if (map) munmap((void *)map, size);
        close(fd);
        return 1;
    }
    if (format < 0) format = size && map[0] == '@' ? FK_FORMAT_FASTQ : FK_FORMAT_FASTA;
    if (format != FK_FORMAT_FASTA && fk_set_input_format(ctx, format, (int32_t)min_qual, (int32_t)qual_off) != FK_OK) {
        fprintf(stderr, "invalid configuration: %s\n", fk_last_error());
        fk_destroy(ctx);
        if (map) munmap((void *)map, size);
        close(fd);
        return 1;
    }
    const size_t window = (size_t)256 << 20;
    auto t0 = std::chrono::steady_clock::now();
    int rc = fk_ingest_reserve(ctx, size);
    for (size_t off = 0; rc == FK_OK && (off < size || off == 0);) {
        const size_t len = std::min(window, size - off);
        rc = fk_ingest(ctx, map ? map + off : nullptr, len, off + len >= size ? 1 : 0);
        off += len;
        if (size == 0) break;
    }
    if (rc == FK_OK) rc = fk_finish(ctx);
    auto t1 = std::chrono::steady_clock::now();
    if (map) munmap((void *)map, size);
    close(fd);
    if (rc != FK_OK) {
        fprintf(stderr, "fk_finish: %s\n", fk_last_error());
        fk_destroy(ctx);
        return 1;
    }
    fk_stats st;
    fk_get_stats(ctx, &st);
    printf("Finished getSuperKmers. parse %.3f ms, signature %.3f ms, %llu super-k-mers, %llu k-mers\n", st.ms_parse,
           st.ms_signature, (unsigned long long)st.superkmers, (unsigned long long)st.kmers);
    printf("extractKXmers%s ended. partition %.3f ms, count %.3f ms, %llu distinct k-mers, host wall %.3f ms\n",
           cfg.use_ht ? "HT" : "", st.ms_partition, st.ms_count, (unsigned long long)st.distinct,
           std::chrono::duration<double, std::milli>(t1 - t0).count());
    if (cfg.write) {
        const int wrc = ranged ? fk_write_bins_range(ctx, outdir, (uint32_t)min_count, (uint32_t)max_count)
                               : fk_write_bins(ctx, outdir);
        if (wrc != FK_OK) {
            fprintf(stderr, "%s: %s\n", ranged ? "fk_write_bins_range" : "fk_write_bins", fk_last_error());
            fk_destroy(ctx);
            return 1;
        }
        printf("Output written to %s\n", outdir);
    }
    if (has_spec) {
        std::vector<uint64_t> hist((size_t)spec_n, 0);
        if (fk_spectrum(ctx, hist.data(), hist.size(), nullptr) != FK_OK) {
            fprintf(stderr, "fk_spectrum: %s\n", fk_last_error());
            fk_destroy(ctx);
            return 1;
        }
        // the output directory exists only once bin files were written into it
        std::string dir(outdir);
        for (size_t i = 1; i <= dir.size(); ++i)
            if (i == dir.size() || dir[i] == '/') (void)mkdir(dir.substr(0, i).c_str(), 0755);
        const std::string path = dir + (dir.empty() || dir.back() == '/' ? "" : "/") + "spectrum.txt";
        FILE *f = fopen(path.c_str(), "w");
        bool ok = f != nullptr;
        for (size_t c = 1; ok && c < hist.size(); ++c) {
            if (!hist[c]) continue;
            ok = fprintf(f, "%s%zu\t%llu\n", c + 1 == hist.size() ? ">=" : "", c, (unsigned long long)hist[c]) > 0;
        }
        if (f && fclose(f) != 0) ok = false;
        if (!ok) {
            fprintf(stderr, "cannot write %s\n", path.c_str());
            fk_destroy(ctx);
            return 1;
        }
        printf("Spectrum written to %s\n", path.c_str());
    }
    if (save_path) {
        if (fk_save(ctx, save_path) != FK_OK) {
            fprintf(stderr, "FASTKMER_CLI_SAVE: %s\n", fk_last_error());
            fk_destroy(ctx);
            return 1;
        }
        printf("Database written to %s\n", save_path);
    }
    if (reads_path) {
        std::vector<uint8_t> text;
        FILE *in = fopen(reads_path, "rb");
        bool ok = in != nullptr;
        if (ok) {
            uint8_t buf[1 << 16];
            for (size_t got; (got = fread(buf, 1, sizeof(buf), in)) > 0;) text.insert(text.end(), buf, buf + got);
            ok = !ferror(in);
            fclose(in);
        }
        if (!ok) {
            fprintf(stderr, "cannot open %s\n", reads_path);
            fk_destroy(ctx);
            return 1;
        }
        // the reads file is cut as the job's input was (auto picked the job's format above)
        size_t n_reads = 0, n_bases = 0;
        int rrc = fk_reads_csr(text.data(), text.size(), format, (int32_t)min_qual, (int32_t)qual_off, nullptr, 0, nullptr, 0,
                               &n_reads, &n_bases);
        std::vector<uint8_t> bases(n_bases + 1);
        std::vector<uint64_t> offsets(n_reads + 1, 0);
        std::vector<fk_read_stat> stats(n_reads + 1);
        if (rrc == FK_OK)
            rrc = fk_reads_csr(text.data(), text.size(), format, (int32_t)min_qual, (int32_t)qual_off, bases.data(), n_bases,
                               offsets.data(), n_reads, &n_reads, &n_bases);
        if (rrc == FK_OK)
            rrc = fk_read_stats(ctx, bases.data(), offsets.data(), n_reads, (uint32_t)min_count, (uint32_t)max_count,
                                stats.data());
        if (rrc != FK_OK) {
            fprintf(stderr, "FASTKMER_CLI_READS: %s\n", fk_last_error());
            fk_destroy(ctx);
            return 1;
        }
        std::string dir(outdir);
        for (size_t i = 1; i <= dir.size(); ++i)
            if (i == dir.size() || dir[i] == '/') (void)mkdir(dir.substr(0, i).c_str(), 0755);
        const std::string path = dir + (dir.empty() || dir.back() == '/' ? "" : "/") + "read_stats.tsv";
        FILE *f = fopen(path.c_str(), "w");
        ok = f != nullptr;
        for (size_t i = 0; ok && i < n_reads; ++i) {
            const fk_read_stat &st = stats[i];
            ok = fprintf(f, "%zu\t%llu\t%u\t%u\t%u\t%u\t%u\t%llu\n", i, (unsigned long long)(offsets[i + 1] - offsets[i]),
                         st.windows, st.hits, st.min, st.median, st.max, (unsigned long long)st.sum) > 0;
        }
        if (f && fclose(f) != 0) ok = false;
        if (!ok) {
            fprintf(stderr, "cannot write %s\n", path.c_str());
            fk_destroy(ctx);
            return 1;
        }
        printf("Read statistics of %zu reads written to %s\n", n_reads, path.c_str());
    }
    if (compare_path) {
        std::vector<uint8_t> text;
        FILE *in = fopen(compare_path, "rb");
        bool ok = in != nullptr;
        if (ok) {
            uint8_t buf[1 << 16];
            for (size_t got; (got = fread(buf, 1, sizeof(buf), in)) > 0;) text.insert(text.end(), buf, buf + got);
            ok = !ferror(in);
            fclose(in);
        }
        if (!ok) {
            fprintf(stderr, "cannot open %s\n", compare_path);
            fk_destroy(ctx);
            return 1;
        }
        // the second sample is a saved database, or is counted as the job's input was (auto picked the job's
        // format above)
        const bool is_db = text.size() >= 8 && !memcmp(text.data(), "FKMERDB\0", 8);
        fk_ctx *other = nullptr;
        int crc = fk_create(&cfg, &other);
        if (is_db) {
            text.clear();
            if (crc == FK_OK) crc = fk_load(other, compare_path);
        }
        if (crc == FK_OK && !is_db && format != FK_FORMAT_FASTA)
            crc = fk_set_input_format(other, format, (int32_t)min_qual, (int32_t)qual_off);
        if (crc == FK_OK && !is_db) crc = fk_ingest_reserve(other, text.size());
        for (size_t off = 0; crc == FK_OK && !is_db && (off < text.size() || off == 0);) {
            const size_t len = std::min(window, text.size() - off);
            crc = fk_ingest(other, text.empty() ? nullptr : text.data() + off, len, off + len >= text.size() ? 1 : 0);
            off += len;
            if (text.empty()) break;
        }
        if (crc == FK_OK && !is_db) crc = fk_finish(other);
        std::vector<uint64_t> mat((size_t)(cmp_n * cmp_n), 0);
        if (crc == FK_OK) crc = fk_compare(ctx, other, mat.data(), (size_t)cmp_n, (size_t)cmp_n);
        if (crc != FK_OK) {
            fprintf(stderr, "FASTKMER_CLI_COMPARE: %s\n", fk_last_error());
            if (other) fk_destroy(other);
            fk_destroy(ctx);
            return 1;
        }
        fk_destroy(other);
        std::string dir(outdir);
        for (size_t i = 1; i <= dir.size(); ++i)
            if (i == dir.size() || dir[i] == '/') (void)mkdir(dir.substr(0, i).c_str(), 0755);
        const std::string path = dir + (dir.empty() || dir.back() == '/' ? "" : "/") + "compare.tsv";
        FILE *f = fopen(path.c_str(), "w");
        ok = f != nullptr;
        size_t lines = 0;
        for (size_t i = 0; ok && i < mat.size(); ++i) {
            if (!mat[i]) continue;
            ok = fprintf(f, "%zu\t%zu\t%llu\n", i / (size_t)cmp_n, i % (size_t)cmp_n, (unsigned long long)mat[i]) > 0;
            ++lines;
        }
        if (f && fclose(f) != 0) ok = false;
        if (!ok) {
            fprintf(stderr, "cannot write %s\n", path.c_str());
            fk_destroy(ctx);
            return 1;
        }
        printf("Comparison with %s (%zu nonzero entries of %llu x %llu) written to %s\n", compare_path, lines,
               (unsigned long long)cmp_n, (unsigned long long)cmp_n, path.c_str());
    }
    fk_destroy(ctx);
    return 0;
}
