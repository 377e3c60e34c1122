// cli.h -- command-line surface of `bucketmap` (bucket_map/main.cpp:12-123), without Sharg.
//
// Same short/long option names and defaults as the reference.  The three values the reference bakes in
// at compile time through CMake (BM_GENOME_PATH, BM_BUCKET_LEN, BM_BUCKET_NUM; CMakeLists.txt:7-58,
// main.cpp:170) are run-time options here (--genome, --bucket-len, --num-buckets), still honouring the
// same -DBM_* definitions as defaults when the tool is built with them.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <filesystem>
#include <stdexcept>
#include <string>
#include <vector>

namespace bm {

struct cmd_arguments {
    bool only_indexer = false;
    std::filesystem::path fastq_path{};
    std::string index_indicator;
    std::filesystem::path output_sam_path{};
    uint8_t query_seed_length = 12;
    uint8_t index_seed_length = 9;
    unsigned int max_read_length = 300;
    unsigned int mapper_sample_size = 15;
    float mapper_distinguishability_threshold = 0.5f;
    unsigned int average_base_quality = 25;
    float allowed_seed_miss_rate = 0.4f;
    float locator_allowed_indel_rate = 0.02f;
    float locator_sample_size = 10;
    unsigned int locator_quality_threshold = 40;
    float frac_min_hash = 0.25f;
    float max_edit_rate = -1.f;   // --max-edit-rate R (bucketmap_align): only alignments within R * read length edits are
                                  // written; negative = unset, every located candidate is written as before
    bool annotate = false;        // --annotate (bucketmap_align): records on the forward strand with =/X CIGAR, NM and MD
    bool clip = false;            // --clip (bucketmap_align): --annotate's records with low-identity ends soft-clipped (S) and AS
    unsigned int clip_match = 1, clip_penalty = 2;   // --clip-scores M,P (implies --clip): bmv_clip's scores, 1..1024 each
    bool best = false;            // --best (bucketmap_align): one record per read, its best alignment's, with a MAPQ that tells a
                                  // unique hit from a repeat and an X0 tag
    float best_margin = 0.05f;    // --best-margin R (implies --best): alignments within max(1, R * read length) edits of the best
                                  // count towards MAPQ and X0
    bool paired = false;          // --paired (bucketmap_align): the FASTQ file is interleaved, records 2p and 2p + 1 are mates;
                                  // the two are placed together and written with the pair's flags, RNEXT, PNEXT and TLEN
                                  // (implies --best and --annotate)
    unsigned int frag_min = 1, frag_max = 1000;      // --frag-range MIN,MAX (implies --paired): what a proper pair may span
    bool frag_auto = false;       // --frag-auto (implies --paired): the range is learned from every verifier block's own pairs;
                                  // --frag-range is then the range of a block with too few informative pairs
    unsigned int frag_cap = 10000;        // --frag-cap N (implies --frag-auto): the longest span that counts as a fragment, 1 .. 65535
    unsigned int frag_min_pairs = 64;     // --frag-min-pairs N (implies --frag-auto): informative pairs a block needs to learn from
    bool rescue = false;          // --rescue (bucketmap_align, implies --paired): a mate without a proper placement is sought beside
                                  // its partner's alignment (mate rescue) and written with XR:i:1
    float rescue_rate = 0.1f;     // --rescue-rate R (implies --rescue): an anchor may have (uint32_t)(R * its length) edits, and so
                                  // may the rescued mate
    bool clip_overlap = false;    // --clip-overlap (bucketmap_align, implies --paired): where the two records of a pair overlap on
                                  // the reference, both are soft-clipped at one cut so that no base is covered twice (bmv_overlap)
    bool affine = false;          // --affine (bucketmap_align): the written alignments are realigned under affine gap costs beside
                                  // their edit path (bmv_realign); POS, CIGAR, NM and MD are the realigned path's, AS:i its score
                                  // (implies --annotate)
    unsigned int affine_match = 1, affine_mismatch = 4, affine_gap_open = 6, affine_gap_extend = 1;   // --affine-scores A,B,O,E
                                  // (implies --affine), 1..1024 each; the default is the common short-read scale, a choice
    unsigned int affine_band = 16;   // --affine-band W (implies --affine), 1..31: D entries of up to 63 - 2 W bases are realigned
    bool left_align = false;      // --left-align (bucketmap_align): the written alignments' I and D entries are moved to their
                                  // leftmost equivalent place on the forward strand (bmv_leftalign), after --affine's realignment
                                  // and before annotate or clip (implies --annotate)
    bool split = false;           // --split (bucketmap_align): a read that spans a breakpoint is written as one primary record and
                                  // 0x800 supplementary records, tied together by SA:Z tags (bmv_split; implies --clip)
    unsigned long split_min_score = 40;   // --split-min-score N (implies --split), 1..2^31: the clipping score a segment needs
    float split_overlap = 0.5f;   // --split-overlap R (implies --split), 0..1: what two segments may share of the shorter one's
                                  // part of the read; bmv_split takes (uint32_t)(R * 1000) permille
    unsigned int split_max = 8;   // --split-max N (implies --split), 1..16: segments per read
    bool sort = false;            // --sort (-o x.bam only): the records in coordinate order, with a x.bam.bai index beside the file
    unsigned long sort_mem = 2048;   // --sort-mem N (implies --sort), >= 1: MiB of BAM stream sorted in one run on the device; more
                                  // is sorted in runs, which are merged on the host (the files are the same)
    bool markdup = false;         // --markdup (-o x.bam only, implies --sort): duplicate reads are flagged 0x400 on the device before
                                  // the sort (include/bmd.h states the rule: unclipped 5' ends, sum of base qualities)
    std::filesystem::path depth_path{}, coverage_path{};   // --depth FILE / --coverage FILE (-o x.bam only, either implies --sort):
                                  // the per-base depth of the records written as bedGraph runs, and one line per reference of
                                  // reads, covered bases, mean depth, base quality and MAPQ (include/bmc.h states the rule)
    std::filesystem::path pileup_path{};   // --pileup FILE (-o x.bam only, implies --sort, in bucketmap_align --annotate too): per
                                  // base what the written records say, and the table of positions where enough of them disagree
                                  // with the reference (include/bmp.h states the rule)
    unsigned long pileup_min_bq = 13, pileup_min_mapq = 0, pileup_min_alt = 2;   // --pileup-min-bq / -min-mapq / -min-alt N
    unsigned long pileup_min_frac_ppm = 200000;   // --pileup-min-frac F, a decimal in [0, 1] with at most six fractional digits
    std::string pileup_threshold_opt;   // the first of those four given: refused without --pileup and without --vcf
    std::filesystem::path vcf_path{};   // --vcf FILE (-o x.bam only, implies --sort, the pileup counting and, in bucketmap_align,
                                  // --annotate): the diploid genotypes at the pileup's SNV sites as VCF 4.2 (include/bmg.h states
                                  // the rule); the pileup's own file is written only with --pileup
    unsigned long vcf_prior = 30, vcf_min_qual = 20;   // --vcf-prior N (phred, 0..255) / --vcf-min-qual N (phred)
    std::string vcf_sample = "sample";   // --vcf-sample NAME: the sample column's name, no tab or newline
    std::string vcf_opt;          // the first of those three or of the three below given: refused without --vcf
    bool vcf_indels = false;      // --vcf-indels: the VCF also carries the insertions and deletions of the records (include/bmn.h states
                                  // the rule); sites by --pileup-min-mapq / -min-alt / -min-frac.  It does not imply --affine --left-align
    unsigned long vcf_indel_qual = 30, vcf_indel_prior = 40;   // --vcf-indel-qual N (phred, 1..93) / --vcf-indel-prior N (phred, 0..255)
    std::string vcf_indel_opt;    // the first of those two given: refused without --vcf-indels
    std::filesystem::path gvcf_path{};  // --gvcf FILE (-o x.bam only, implies what --vcf implies; with or without --vcf FILE): the calls of
                                  // --vcf and, between them, the hom-ref blocks of every other base as VCF 4.2 (include/bmr.h states the rule)
    std::vector<uint32_t> gvcf_bands{1, 10, 20, 30, 40, 50, 60, 70, 80, 90, 99};   // --gvcf-bands B1,B2,...: the GQ bounds at which a block ends
    bool gvcf_bands_given = false;   // refused without --gvcf
    bool vcf_bias = false;        // --vcf-bias: FS, MQ, ADF and ADR on the SNV lines of --vcf / --gvcf (include/bmb.h states the rule)
    unsigned long vcf_max_fs = 60, vcf_min_mq = 0;   // --vcf-max-fs N (phred, 1..60): FS >= N is StrandBias / --vcf-min-mq N (0..255, 0 is off): MQ < N is LowMQ
    std::string vcf_bias_opt;     // the first of those two given: refused without --vcf-bias
    bool vcf_phase = false;       // --vcf-phase: read-backed phase of the het SNV lines of --vcf / --gvcf (include/bmk.h states the rule)
    unsigned long phase_min_links = 2, phase_min_frac_ppm = 800000, phase_reach = 4;   // --phase-min-links N (>= 1) / --phase-min-frac F (above 0.5, at most 1) / --phase-reach N (1..8)
    std::string phase_opt;        // the first of those three given: refused without --vcf-phase
    std::filesystem::path stats_path{};   // --stats FILE (-o x.bam only, implies --sort): the mapping statistics of the records written (include/bmq.h states the rule)
    unsigned long stats_max_cycle = 1024, stats_max_insert = 8000;   // --stats-max-cycle N / --stats-max-insert N (1..65535): the rows of the per-cycle tables / of the insert sizes
    std::string stats_opt;        // the first of those two given: refused without --stats
    // run-time replacements of the compile-time configuration
#ifdef BM_GENOME_PATH
    std::filesystem::path genome_path = BM_GENOME_PATH;
#else
    std::filesystem::path genome_path{};
#endif
#ifdef BM_BUCKET_LEN
    unsigned int bucket_len = BM_BUCKET_LEN;
#else
    unsigned int bucket_len = 65536;
#endif
#ifdef BM_BUCKET_NUM
    unsigned int num_buckets = BM_BUCKET_NUM;
#else
    unsigned int num_buckets = 0;   // 0 = the CMake awk rule applied to --genome
#endif
    std::vector<int> gpus{0};
    uint64_t hash_seed = 20240004;
    unsigned int host_threads = 0;
    bool early_exit = true;    // BMF_FLAG_EARLY_EXIT (identical output, fewer index rows read); --no-early-exit
                               // makes the filter read every row the reference reads
    int gpu_index = -1;        // index rows built on the device (identical files): 1 = --gpu-index, 0 = --host-index,
                               // -1 = on the device where its kernels cover the seed length (3 <= -k <= 10)
};

struct parser_error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

inline std::vector<int> parse_gpu_list(const std::string &v) {
    std::vector<int> out;
    if (v.find(',') == std::string::npos && !v.empty()) {
        // a single number N means devices 0..N-1 when prefixed with 'n', otherwise device id
        if (v[0] == 'n') {
            for (int i = 0; i < std::atoi(v.c_str() + 1); i++) out.push_back(i);
            return out;
        }
    }
    size_t pos = 0;
    while (pos <= v.size()) {
        size_t c = v.find(',', pos);
        if (c == std::string::npos) c = v.size();
        if (c > pos) out.push_back(std::atoi(v.substr(pos, c - pos).c_str()));
        pos = c + 1;
    }
    if (out.empty()) throw parser_error("--gpus needs a device list such as 0,1,2,3 or n8");
    return out;
}

// --pileup-min-frac: a decimal in [0, 1] with at most six fractional digits ("0", "1", "0.2", "0.000001", "1.000000"), as
// parts per million, without floating point; false for everything else (a sign, an exponent, seven digits, above 1)
inline bool parse_ppm(const std::string &s, unsigned long &ppm) {
    size_t at = 0;
    while (at < s.size() && s[at] >= '0' && s[at] <= '9') at++;
    if (at == 0 || at > 1 || s[0] > '1') return false;   // one digit before the point: 0 or 1
    unsigned long v = static_cast<unsigned long>(s[0] - '0') * 1000000ul;
    if (at < s.size()) {
        if (s[at] != '.' || s.size() - at - 1 < 1 || s.size() - at - 1 > 6) return false;
        unsigned long scale = 100000ul;
        for (size_t k = at + 1; k < s.size(); k++, scale /= 10) {
            if (s[k] < '0' || s[k] > '9') return false;
            v += static_cast<unsigned long>(s[k] - '0') * scale;
        }
    }
    if (v > 1000000ul) return false;
    ppm = v;
    return true;
}

// Parses argv like sharg does for these options: `-k 9`, `--index-seed 9`, `--index-seed=9`.
inline cmd_arguments parse_arguments(int argc, char **argv) {
    cmd_arguments a;
    bool have_indicator = false;
    auto has_ext = [](const std::filesystem::path &p, std::initializer_list<const char *> exts) {
        std::string e = p.extension().string();
        if (!e.empty()) e.erase(0, 1);
        for (auto x : exts)
            if (e == x) return true;
        return false;
    };
    for (int i = 1; i < argc; i++) {
        std::string opt = argv[i], val;
        bool inline_val = false;
        if (opt.rfind("--", 0) == 0) {
            size_t eq = opt.find('=');
            if (eq != std::string::npos) {
                val = opt.substr(eq + 1);
                opt = opt.substr(0, eq);
                inline_val = true;
            }
        }
        auto value = [&]() -> std::string {
            if (inline_val) return val;
            if (i + 1 >= argc) throw parser_error("Missing value for option " + opt + ".");
            return argv[++i];
        };
        auto as_uint = [&](const std::string &s) -> unsigned long {
            char *end = nullptr;
            unsigned long v = std::strtoul(s.c_str(), &end, 10);
            if (s.empty() || *end) throw parser_error("Value parse failed for " + opt + ": Argument " + s + " could not be parsed as a number.");
            return v;
        };
        auto as_float = [&](const std::string &s) -> float {
            char *end = nullptr;
            float v = std::strtof(s.c_str(), &end);
            if (s.empty() || *end) throw parser_error("Value parse failed for " + opt + ": Argument " + s + " could not be parsed as a number.");
            return v;
        };
        if (opt == "-x" || opt == "--run-index") a.only_indexer = true;
        else if (opt == "-q" || opt == "--query-file") {
            a.fastq_path = value();
            // x.fq.gz / x.fastq.gz: BGZF (bgzf_in.h); the extension below .gz decides as before
            if (!has_ext(a.fastq_path.extension() == ".gz" ? a.fastq_path.stem() : a.fastq_path, {"fq", "fastq"}))
                throw parser_error("Validation failed for option -q/--query-file: Expected one of the following valid extensions: [fq, fastq]!");
            if (!std::filesystem::exists(a.fastq_path))
                throw parser_error("Validation failed for option -q/--query-file: The file " + a.fastq_path.string() + " does not exist!");
        } else if (opt == "-i" || opt == "--index-indicator") { a.index_indicator = value(); have_indicator = true; }
        else if (opt == "-o" || opt == "--output-file") {
            a.output_sam_path = value();
            if (!has_ext(a.output_sam_path, {"sam", "bam"}))   // the extension decides: SAM text, or BAM (BGZF blocks, bmz.h)
                throw parser_error("Validation failed for option -o/--output-file: Expected one of the following valid extensions: [sam, bam]!");
            if (std::filesystem::exists(a.output_sam_path))
                throw parser_error("Validation failed for option -o/--output-file: The file " + a.output_sam_path.string() + " already exists!");
        } else if (opt == "-k" || opt == "--index-seed") a.index_seed_length = static_cast<uint8_t>(as_uint(value()));
        else if (opt == "-b" || opt == "--average-base-quality") a.average_base_quality = static_cast<unsigned>(as_uint(value()));
        else if (opt == "-l" || opt == "--query-seed") a.query_seed_length = static_cast<uint8_t>(as_uint(value()));
        else if (opt == "-r" || opt == "--read-len") a.max_read_length = static_cast<unsigned>(as_uint(value()));
        else if (opt == "-s" || opt == "--mapper-samples") a.mapper_sample_size = static_cast<unsigned>(as_uint(value()));
        else if (opt == "-d" || opt == "--distinguishability") a.mapper_distinguishability_threshold = as_float(value());
        else if (opt == "-e" || opt == "--max-error-rate") a.allowed_seed_miss_rate = as_float(value());
        else if (opt == "-n" || opt == "--max-indel-rate") a.locator_allowed_indel_rate = as_float(value());
        else if (opt == "-p" || opt == "--locator-samples") a.locator_sample_size = as_float(value());
        else if (opt == "-u" || opt == "--quality") a.locator_quality_threshold = static_cast<unsigned>(as_uint(value()));
        else if (opt == "-f" || opt == "--kmer-frac") a.frac_min_hash = as_float(value());
        else if (opt == "--max-edit-rate") {
            const std::string s = value();
            a.max_edit_rate = as_float(s);
            if (!(a.max_edit_rate >= 0.f)) throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a number >= 0.");
        }
        else if (opt == "--annotate") a.annotate = true;
        else if (opt == "--best") a.best = true;
        else if (opt == "--best-margin") {
            const std::string s = value();
            a.best_margin = as_float(s);
            if (!(a.best_margin >= 0.f)) throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a number >= 0.");
            a.best = true;
        }
        else if (opt == "--clip") a.clip = true;
#ifdef BM_ALIGN
        else if (opt == "--paired") a.paired = true;
        else if (opt == "--frag-range") {
            const std::string s = value();
            const size_t comma = s.find(',');
            if (comma == std::string::npos) throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be MIN,MAX such as 1,1000.");
            const unsigned long lo = as_uint(s.substr(0, comma)), hi = as_uint(s.substr(comma + 1));
            if (lo > hi || hi > 0xFFFFFFFFul)
                throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be two numbers MIN <= MAX below 2^32.");
            a.frag_min = static_cast<unsigned>(lo);
            a.frag_max = static_cast<unsigned>(hi);
            a.paired = true;
        }
        else if (opt == "--frag-auto") a.frag_auto = a.paired = true;
        else if (opt == "--frag-cap") {
            const std::string s = value();
            const unsigned long v = as_uint(s);
            if (v < 1 || v > 65535) throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a number in 1..65535.");
            a.frag_cap = static_cast<unsigned>(v);
            a.frag_auto = a.paired = true;
        }
        else if (opt == "--frag-min-pairs") {
            const std::string s = value();
            const unsigned long v = as_uint(s);
            if (v > 0xFFFFFFFFul) throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a number below 2^32.");
            a.frag_min_pairs = static_cast<unsigned>(v);
            a.frag_auto = a.paired = true;
        }
        else if (opt == "--rescue") a.rescue = true;
        else if (opt == "--rescue-rate") {
            const std::string s = value();
            char *end = nullptr;
            const float r = std::strtof(s.c_str(), &end);
            if (s.empty() || *end != '\0' || !(r >= 0.f) || r > 1.f)
                throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a rate between 0 and 1.");
            a.rescue_rate = r;
            a.rescue = true;
        }
        else if (opt == "--clip-overlap") a.clip_overlap = a.paired = true;
        else if (opt == "--affine") a.affine = true;
        else if (opt == "--affine-scores") {
            const std::string s = value();
            unsigned long v[4] = {0, 0, 0, 0};
            size_t pos = 0;
            for (int f = 0; f < 4; f++) {
                const size_t comma = f < 3 ? s.find(',', pos) : s.size();
                if (comma == std::string::npos || (f == 3 && s.find(',', pos) != std::string::npos))
                    throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be A,B,O,E such as 1,4,6,1.");
                v[f] = as_uint(s.substr(pos, comma - pos));
                if (v[f] < 1 || v[f] > 1024) throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be four numbers in 1..1024.");
                pos = comma + 1;
            }
            a.affine_match = static_cast<unsigned>(v[0]);
            a.affine_mismatch = static_cast<unsigned>(v[1]);
            a.affine_gap_open = static_cast<unsigned>(v[2]);
            a.affine_gap_extend = static_cast<unsigned>(v[3]);
            a.affine = true;
        }
        else if (opt == "--affine-band") {
            const std::string s = value();
            const unsigned long w = as_uint(s);
            if (w < 1 || w > 31) throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a number in 1..31.");
            a.affine_band = static_cast<unsigned>(w);
            a.affine = true;
        }
        else if (opt == "--left-align") a.left_align = true;
        else if (opt == "--split") a.split = true;
        else if (opt == "--split-min-score") {
            const std::string s = value();
            const unsigned long v = as_uint(s);
            if (v < 1 || v > 0x80000000ul) throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a number in 1..2^31.");
            a.split_min_score = v;
            a.split = true;
        }
        else if (opt == "--split-overlap") {
            const std::string s = value();
            const float r = as_float(s);
            if (!(r >= 0.f) || r > 1.f) throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a rate between 0 and 1.");
            a.split_overlap = r;
            a.split = true;
        }
        else if (opt == "--split-max") {
            const std::string s = value();
            const unsigned long v = as_uint(s);
            if (v < 1 || v > 16) throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a number in 1..16.");
            a.split_max = static_cast<unsigned>(v);
            a.split = true;
        }
#else
        else if (opt == "--split" || opt == "--split-min-score" || opt == "--split-overlap" || opt == "--split-max")
            throw parser_error("Option " + opt + " belongs to bucketmap_align: this tool does not align, so it has no alignments to split.");
        else if (opt == "--left-align")
            throw parser_error("Option " + opt + " belongs to bucketmap_align: this tool does not align, so it has no indels to normalise.");
        else if (opt == "--affine" || opt == "--affine-scores" || opt == "--affine-band")
            throw parser_error("Option " + opt + " belongs to bucketmap_align: this tool does not align, so it has nothing to realign.");
        else if (opt == "--paired" || opt == "--frag-range" || opt == "--frag-auto" || opt == "--frag-cap" || opt == "--frag-min-pairs" ||
                 opt == "--rescue" || opt == "--rescue-rate" || opt == "--clip-overlap")
            throw parser_error("Option " + opt + " belongs to bucketmap_align: this tool does not align, so it cannot place mates together.");
#endif
        else if (opt == "--clip-scores") {
            const std::string s = value();
            const size_t comma = s.find(',');
            if (comma == std::string::npos) throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be M,P such as 1,2.");
            a.clip_match = static_cast<unsigned>(as_uint(s.substr(0, comma)));
            a.clip_penalty = static_cast<unsigned>(as_uint(s.substr(comma + 1)));
            if (a.clip_match < 1 || a.clip_match > 1024 || a.clip_penalty < 1 || a.clip_penalty > 1024)
                throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be two numbers in 1..1024.");
            a.clip = true;
        }
        else if (opt == "--sort") a.sort = true;
        else if (opt == "--sort-mem") {
            const std::string s = value();
            const unsigned long v = as_uint(s);
            if (v < 1 || v > (1ul << 24)) throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a number of MiB in 1..2^24.");
            a.sort_mem = v;
            a.sort = true;
        }
        else if (opt == "--markdup") a.markdup = a.sort = true;
        else if (opt == "--depth" || opt == "--coverage") {
            (opt == "--depth" ? a.depth_path : a.coverage_path) = value();
            a.sort = true;
        }
        else if (opt == "--stats") {
            a.stats_path = value();
            a.sort = true;
        }
        else if (opt == "--stats-max-cycle" || opt == "--stats-max-insert") {
            const std::string s = value();
            const unsigned long v = as_uint(s);
            if (s[0] < '0' || s[0] > '9' || v < 1 || v > 65535ul)
                throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a number in 1..65535.");
            (opt == "--stats-max-cycle" ? a.stats_max_cycle : a.stats_max_insert) = v;
            if (a.stats_opt.empty()) a.stats_opt = opt;
        }
        else if (opt == "--pileup") {
            a.pileup_path = value();
            a.sort = true;
        }
        else if (opt == "--pileup-min-bq" || opt == "--pileup-min-mapq" || opt == "--pileup-min-alt") {
            const std::string s = value();
            const unsigned long v = as_uint(s);
            const bool alt = opt == "--pileup-min-alt";
            if (s[0] < '0' || s[0] > '9' || v > 0xFFFFFFFFul || (alt && v < 1))
                throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a number in " + (alt ? "1" : "0") + "..2^32-1.");
            (alt ? a.pileup_min_alt : opt == "--pileup-min-bq" ? a.pileup_min_bq : a.pileup_min_mapq) = v;
            if (a.pileup_threshold_opt.empty()) a.pileup_threshold_opt = opt;
        }
        else if (opt == "--pileup-min-frac") {
            const std::string s = value();
            if (!parse_ppm(s, a.pileup_min_frac_ppm))
                throw parser_error("Value parse failed for " + opt + ": Argument " + s +
                                   " must be a decimal between 0 and 1 with at most six fractional digits, such as 0.2.");
            if (a.pileup_threshold_opt.empty()) a.pileup_threshold_opt = opt;
        }
        else if (opt == "--vcf") {
            a.vcf_path = value();
            a.sort = true;
        }
        else if (opt == "--vcf-prior" || opt == "--vcf-min-qual") {
            const std::string s = value();
            const unsigned long v = as_uint(s);
            const bool prior = opt == "--vcf-prior";
            if (s[0] < '0' || s[0] > '9' || v > (prior ? 255ul : 0xFFFFFFFFul / 100))
                throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a number in 0.." + (prior ? "255" : "42949672") + ".");
            (prior ? a.vcf_prior : a.vcf_min_qual) = v;
            if (a.vcf_opt.empty()) a.vcf_opt = opt;
        }
        else if (opt == "--vcf-indels") {
            a.vcf_indels = true;
            if (a.vcf_opt.empty()) a.vcf_opt = opt;
        }
        else if (opt == "--vcf-indel-qual" || opt == "--vcf-indel-prior") {
            const std::string s = value();
            const unsigned long v = as_uint(s);
            const bool prior = opt == "--vcf-indel-prior";
            if (s[0] < '0' || s[0] > '9' || v > (prior ? 255ul : 93ul) || (!prior && v == 0))
                throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a number in " + (prior ? "0..255" : "1..93") + ".");
            (prior ? a.vcf_indel_prior : a.vcf_indel_qual) = v;
            if (a.vcf_opt.empty()) a.vcf_opt = opt;
            if (a.vcf_indel_opt.empty()) a.vcf_indel_opt = opt;
        }
        else if (opt == "--vcf-bias") {
            a.vcf_bias = true;
        }
        else if (opt == "--vcf-max-fs" || opt == "--vcf-min-mq") {
            const std::string s = value();
            const unsigned long v = as_uint(s);
            const bool fs = opt == "--vcf-max-fs";
            if (s[0] < '0' || s[0] > '9' || v > (fs ? 60ul : 255ul) || (fs && v == 0))
                throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a number in " + (fs ? "1..60" : "0..255") + ".");
            (fs ? a.vcf_max_fs : a.vcf_min_mq) = v;
            if (a.vcf_bias_opt.empty()) a.vcf_bias_opt = opt;
        }
        else if (opt == "--vcf-phase") {
            a.vcf_phase = true;
        }
        else if (opt == "--phase-min-links" || opt == "--phase-reach") {
            const std::string s = value();
            const unsigned long v = as_uint(s);
            const bool reach = opt == "--phase-reach";
            if (s[0] < '0' || s[0] > '9' || v < 1 || v > (reach ? 8ul : 0xFFFFFFFFul))
                throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be a number in " + (reach ? "1..8" : "1..2^32-1") + ".");
            (reach ? a.phase_reach : a.phase_min_links) = v;
            if (a.phase_opt.empty()) a.phase_opt = opt;
        }
        else if (opt == "--phase-min-frac") {
            const std::string s = value();
            unsigned long ppm = 0;
            if (!parse_ppm(s, ppm) || ppm < 500001ul)
                throw parser_error("Value parse failed for " + opt + ": Argument " + s +
                                   " must be a decimal above 0.5 and at most 1 with at most six fractional digits, such as 0.8.");
            a.phase_min_frac_ppm = ppm;
            if (a.phase_opt.empty()) a.phase_opt = opt;
        }
        else if (opt == "--gvcf") {
            a.gvcf_path = value();
            a.sort = true;
        }
        else if (opt == "--gvcf-bands") {
            const std::string s = value();
            std::vector<uint32_t> bands;
            bool good = !s.empty();
            for (size_t at = 0; good && at <= s.size();) {
                const size_t e = std::min(s.find(',', at), s.size());
                unsigned long v = 0;
                good = e > at && e - at <= 2;
                for (size_t k = at; good && k < e; k++) good = s[k] >= '0' && s[k] <= '9', v = 10 * v + static_cast<unsigned long>(s[k] - '0');
                good = good && v >= 1 && v <= 99 && (bands.empty() || v > bands.back()) && bands.size() < 16;
                if (good) bands.push_back(static_cast<uint32_t>(v));
                at = e + 1;
            }
            if (!good)
                throw parser_error("Value parse failed for " + opt + ": Argument " + s + " must be at most 16 ascending numbers in 1..99 with commas between them, such as 20,60.");
            a.gvcf_bands = bands;
            a.gvcf_bands_given = true;
        }
        else if (opt == "--vcf-sample") {
            a.vcf_sample = value();
            if (a.vcf_sample.empty() || a.vcf_sample.find_first_of("\t\n\r") != std::string::npos)
                throw parser_error("Value parse failed for " + opt + ": a sample name is not empty and holds no tab or newline.");
            if (a.vcf_opt.empty()) a.vcf_opt = opt;
        }
        else if (opt == "--version-check") (void)value();   // Sharg built-in used by the benchmark scripts
        else if (opt == "--genome") a.genome_path = value();
        else if (opt == "--bucket-len") a.bucket_len = static_cast<unsigned>(as_uint(value()));
        else if (opt == "--num-buckets") a.num_buckets = static_cast<unsigned>(as_uint(value()));
        else if (opt == "--gpus") a.gpus = parse_gpu_list(value());
        else if (opt == "--hash-seed") a.hash_seed = as_uint(value());
        else if (opt == "--early-exit") a.early_exit = true;
        else if (opt == "--no-early-exit") a.early_exit = false;
        else if (opt == "--gpu-index") a.gpu_index = 1;
        else if (opt == "--host-index") a.gpu_index = 0;
        else if (opt == "--threads") a.host_threads = static_cast<unsigned>(as_uint(value()));
        else throw parser_error("Unknown option " + opt + ". In case this is meant to be a non-option/argument/parameter, please specify the start of non-options with '--'.");
    }
    if (!have_indicator) throw parser_error("Option -i/--index-indicator is required but not set.");
    if (a.split && (a.best || a.paired || a.rescue || a.max_edit_rate >= 0.f))
        throw parser_error(std::string("Option --split cannot be combined with ") +
                           (a.clip_overlap ? "--clip-overlap" : a.rescue ? "--rescue" : a.frag_auto ? "--frag-auto" : a.paired ? "--paired" : a.best ? "--best" : "--max-edit-rate") +
                           ": they judge a read by the edits of one end-to-end alignment, which mean nothing for a read that "
                           "spans a breakpoint.");
    if (a.sort && !a.output_sam_path.empty() && a.output_sam_path.extension() != ".bam") {
        std::filesystem::path bam = a.output_sam_path;
        bam.replace_extension(".bam");
        throw parser_error(std::string("Validation failed for option ") +
                           (!a.depth_path.empty() ? "--depth" : !a.coverage_path.empty() ? "--coverage" : !a.pileup_path.empty() ? "--pileup" :
                            !a.vcf_path.empty() ? "--vcf" : !a.gvcf_path.empty() ? "--gvcf" : a.markdup ? "--markdup" : !a.stats_path.empty() ? "--stats" : "--sort") +
                           ": only BAM output is sorted and indexed; write -o " + bam.string() + " instead of -o " +
                           a.output_sam_path.string() + ".");
    }
    if (!a.pileup_threshold_opt.empty() && a.pileup_path.empty() && a.vcf_path.empty() && a.gvcf_path.empty())
        throw parser_error("Validation failed for option " + a.pileup_threshold_opt + ": it is a threshold of --pileup FILE, which is not given.");
    if (!a.pileup_path.empty() && a.output_sam_path.empty() && !a.only_indexer)
        throw parser_error("Validation failed for option --pileup: the pileup is that of the records of a sorted BAM file; name one with -o x.bam.");
    if (!a.pileup_path.empty() && (a.pileup_path == a.depth_path || a.pileup_path == a.coverage_path))
        throw parser_error("Validation failed for option --pileup: " + a.pileup_path.string() + " is the file of " +
                           (a.pileup_path == a.depth_path ? "--depth" : "--coverage") + " too.");
    if (!a.vcf_opt.empty() && a.vcf_path.empty() && a.gvcf_path.empty())
        throw parser_error("Validation failed for option " + a.vcf_opt + ": it is an option of --vcf FILE, which is not given.");
    if (a.vcf_bias && a.vcf_path.empty() && a.gvcf_path.empty())
        throw parser_error("Validation failed for option --vcf-bias: it annotates the lines of --vcf FILE or --gvcf FILE, neither is given.");
    if (!a.vcf_bias_opt.empty() && !a.vcf_bias)
        throw parser_error("Validation failed for option " + a.vcf_bias_opt + ": it is an option of --vcf-bias, which is not given.");
    if (a.vcf_phase && a.vcf_path.empty() && a.gvcf_path.empty())
        throw parser_error("Validation failed for option --vcf-phase: it phases the het lines of --vcf FILE or --gvcf FILE, neither is given.");
    if (!a.phase_opt.empty() && !a.vcf_phase)
        throw parser_error("Validation failed for option " + a.phase_opt + ": it is an option of --vcf-phase, which is not given.");
    if (!a.vcf_indel_opt.empty() && !a.vcf_indels)
        throw parser_error("Validation failed for option " + a.vcf_indel_opt + ": it is an option of --vcf-indels, which is not given.");
    if (!a.vcf_path.empty() && a.output_sam_path.empty() && !a.only_indexer)
        throw parser_error("Validation failed for option --vcf: the genotypes are those of the records of a sorted BAM file; name one with -o x.bam.");
    if (!a.vcf_path.empty() && (a.vcf_path == a.pileup_path || a.vcf_path == a.depth_path || a.vcf_path == a.coverage_path))
        throw parser_error("Validation failed for option --vcf: " + a.vcf_path.string() + " is the file of " +
                           (a.vcf_path == a.pileup_path ? "--pileup" : a.vcf_path == a.depth_path ? "--depth" : "--coverage") + " too.");
    if (a.gvcf_bands_given && a.gvcf_path.empty())
        throw parser_error("Validation failed for option --gvcf-bands: it is an option of --gvcf FILE, which is not given.");
    if (!a.gvcf_path.empty() && a.output_sam_path.empty() && !a.only_indexer)
        throw parser_error("Validation failed for option --gvcf: the genotypes are those of the records of a sorted BAM file; name one with -o x.bam.");
    if (!a.gvcf_path.empty() && (a.gvcf_path == a.vcf_path || a.gvcf_path == a.pileup_path || a.gvcf_path == a.depth_path || a.gvcf_path == a.coverage_path))
        throw parser_error("Validation failed for option --gvcf: " + a.gvcf_path.string() + " is the file of " +
                           (a.gvcf_path == a.vcf_path ? "--vcf" : a.gvcf_path == a.pileup_path ? "--pileup" : a.gvcf_path == a.depth_path ? "--depth" : "--coverage") + " too.");
    if ((!a.depth_path.empty() || !a.coverage_path.empty()) && a.output_sam_path.empty() && !a.only_indexer)
        throw parser_error(std::string("Validation failed for option ") + (!a.depth_path.empty() ? "--depth" : "--coverage") +
                           ": depth and coverage are those of the records of a sorted BAM file; name one with -o x.bam.");
    if (!a.depth_path.empty() && a.depth_path == a.coverage_path)
        throw parser_error("Validation failed for option --coverage: " + a.coverage_path.string() + " is the file of --depth too.");
    if (!a.stats_opt.empty() && a.stats_path.empty())
        throw parser_error("Validation failed for option " + a.stats_opt + ": it is an option of --stats FILE, which is not given.");
    if (!a.stats_path.empty() && a.output_sam_path.empty() && !a.only_indexer)
        throw parser_error("Validation failed for option --stats: the statistics are those of the records of a sorted BAM file; name one with -o x.bam.");
    if (!a.stats_path.empty() && (a.stats_path == a.depth_path || a.stats_path == a.coverage_path || a.stats_path == a.pileup_path || a.stats_path == a.vcf_path ||
                                  a.stats_path == a.gvcf_path))
        throw parser_error("Validation failed for option --stats: " + a.stats_path.string() + " is the file of " +
                           (a.stats_path == a.depth_path ? "--depth" : a.stats_path == a.coverage_path ? "--coverage" : a.stats_path == a.pileup_path ? "--pileup" :
                            a.stats_path == a.vcf_path ? "--vcf" : "--gvcf") + " too.");
    if (a.split) a.clip = a.annotate = true;
    if (a.rescue) a.paired = true;
    if (a.paired) a.best = a.annotate = true;
    if (a.affine || a.left_align) a.annotate = true;
#ifdef BM_ALIGN
    if (!a.pileup_path.empty() || !a.vcf_path.empty() || !a.gvcf_path.empty()) a.annotate = true;   // the reference's own record layout is not forward-strand: a pileup over it would be wrong
#endif
    return a;
}

}  // namespace bm
