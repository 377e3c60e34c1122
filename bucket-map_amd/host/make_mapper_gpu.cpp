// make_mapper_gpu.cpp -- the product's factories: the MI355X filter behind bm::mapper and the MI355X
// locator scan behind bm::offset_scanner.
// (main.cpp:202-209: q_gram_mapper<BM_BUCKET_NUM> map(BM_BUCKET_LEN, read_len, k, q, S, fault, d, b))
#include "../../include/bmc.h"
#include "../../include/bmp.h"
#include "../../include/bmg.h"
#include "../../include/bmn.h"
#include "../../include/bmr.h"
#include "../../include/bmb.h"
#include "../../include/bmk.h"
#include "../../include/bmq.h"
#include "../../include/bmd.h"
#include "../../include/bms.h"
#include "../../include/bmz.h"
#include "bgzf.h"
#include "bm_indexer.h"
#include "cli.h"
#include "gpu_alignment_verifier.h"
#include "gpu_block_inflater.h"
#include "gpu_offset_scanner.h"
#include "gpu_q_gram_mapper.h"

#include <sys/resource.h>

#include <memory>
#include <thread>

// HIP's start-up and the loading of the library's code objects take 0.2-0.4 s in a fresh process: a throw-away filter
// context on every device of --gpus pays for them while main() reads the FASTA file (tools/init_probe.py).
std::thread bm_warm_up(const bm::cmd_arguments &args) {
    std::vector<int> devices = args.gpus.empty() ? std::vector<int>{0} : args.gpus;
    std::sort(devices.begin(), devices.end());
    devices.erase(std::unique(devices.begin(), devices.end()), devices.end());
    return std::thread([devices] {
        for (int d : devices) {
            bmf_params p{};
            p.num_buckets = 64;
            p.q = 4;
            p.k = 4;
            p.num_samples = 1;
            p.num_fault = 1;
            p.max_candidates = 30;
            p.read_len = 32;
            p.num_segment_samples = 5;
            p.device = d;
            bmf_ctx *ctx = nullptr;
            if (bmf_create(&p, &ctx) == BMF_OK) bmf_destroy(ctx);
        }
    });
}

std::unique_ptr<bm::mapper> bm_make_mapper(const bm::cmd_arguments &args, unsigned int num_buckets, unsigned int fault) {
    return std::make_unique<bm::gpu_q_gram_mapper>(num_buckets, args.bucket_len, args.max_read_length,
                                                   args.query_seed_length, args.index_seed_length,
                                                   args.mapper_sample_size, fault,
                                                   args.mapper_distinguishability_threshold, args.average_base_quality,
                                                   30, 5, args.gpus, args.early_exit ? BMF_FLAG_EARLY_EXIT : 0u);
}

// --gpu-index: bucket_indexer::index on the device (bmf_build_index), rows copied back for the files.
bool bm_gpu_index(const bm::cmd_arguments &args, const bm::Genome &genome, unsigned int num_buckets, bm::QgramIndex &ix) {
    ix = bm::QgramIndex();
    ix.num_buckets = num_buckets;
    ix.row_bytes = (num_buckets + 7u) >> 3;
    bm::select_qgrams(ix, args.index_seed_length, bm::FracMinHash::from_seed(args.hash_seed), args.frac_min_hash);
    const std::vector<bm::Bucket> buckets = bm::cut_buckets(genome, static_cast<int>(args.bucket_len), static_cast<int>(args.max_read_length));
    std::vector<uint64_t> rec_off(genome.seqs.size() + 1, 0);
    for (size_t r = 0; r < genome.seqs.size(); r++) rec_off[r + 1] = rec_off[r] + genome.seqs[r].size();
    std::vector<uint8_t> flat(rec_off.back());
    for (size_t r = 0; r < genome.seqs.size(); r++)
        std::copy(genome.seqs[r].begin(), genome.seqs[r].end(), flat.begin() + static_cast<std::ptrdiff_t>(rec_off[r]));
    std::vector<uint64_t> bstart(buckets.size());
    std::vector<uint32_t> blen(buckets.size());
    for (size_t b = 0; b < buckets.size(); b++) {
        bstart[b] = rec_off[buckets[b].record] + buckets[b].start;
        blen[b] = buckets[b].end - buckets[b].start;
        ix.bucket_id.push_back(genome.ids[buckets[b].record]);
    }
    bmf_params p{};
    p.num_buckets = num_buckets;
    p.q = args.index_seed_length;
    // the index rows depend on q and the buckets only: the mapper's own limits (read_len, k - q + 1 ...) must not
    // decide whether an index can be BUILT, so the build context asks for the smallest mapper there is
    p.k = args.index_seed_length;
    p.num_samples = 1;
    p.num_fault = 1;
    p.max_candidates = 1;
    p.read_len = args.index_seed_length;
    p.num_segment_samples = 5;
    p.device = args.gpus.front();
    bmf_ctx *c = nullptr;
    int rc = bmf_create(&p, &c);
    if (rc == BMF_ERR_UNSUPPORTED || rc == BMF_ERR_ARG) return false;   // not a geometry the device build covers: host indexer
    if (rc != BMF_OK) throw std::runtime_error(std::string("--gpu-index: ") + bmf_last_error());
    rc = bmf_build_index(c, flat.data(), flat.size(), bstart.data(), blen.data(), static_cast<uint32_t>(buckets.size()),
                         ix.kmer_to_index.data(), ix.kmer_to_index.size());
    if (rc == BMF_ERR_UNSUPPORTED) {
        bmf_destroy(c);
        return false;
    }
    if (rc == BMF_OK) {
        ix.rows.assign(static_cast<size_t>(ix.num_rows) * ix.row_bytes, 0);
        rc = bmf_index_download(c, ix.rows.data(), nullptr);
    }
    const std::string why = rc == BMF_OK ? "" : bmf_last_error();
    bmf_destroy(c);
    if (rc != BMF_OK) throw std::runtime_error("--gpu-index: " + why);
    return true;
}

std::unique_ptr<bm::offset_scanner> bm_make_scanner(const bm::cmd_arguments &args, int allowed_mismatch, int allowed_indel) {
    return std::make_unique<bm::gpu_offset_scanner>(args.query_seed_length, static_cast<uint32_t>(args.locator_sample_size),
                                                    allowed_mismatch, allowed_indel,
                                                    args.bucket_len + args.max_read_length, args.gpus);
}

std::unique_ptr<bm::alignment_verifier> bm_make_verifier(const bm::cmd_arguments &args) {
    return std::make_unique<bm::gpu_alignment_verifier>(args.gpus);
}

// -o x.bam: the BGZF blocks of the BAM stream are deflated on the first device of --gpus (bmz_deflate; the rule and so
// the bytes are those of host/bgzf.h).  No host fall-back: a failing device call ends the run.
namespace {
class gpu_block_compressor : public bm::block_compressor {
    bmz_ctx *ctx_ = nullptr;

public:
    explicit gpu_block_compressor(int device) : device_(device) {
        if (bmz_create(device, &ctx_) != BMZ_OK) throw std::runtime_error(std::string("bmz_create: ") + bmz_last_error());
    }
    ~gpu_block_compressor() override {
        bmr_destroy(blocks_);
        bmq_destroy(stats_);
        bmk_destroy(phase_);
        bmb_destroy(bias_);
        bmn_destroy(indel_);
        bmg_destroy(geno_);
        bmp_destroy(pile_);
        bmc_destroy(cover_);
        bmd_destroy(mark_);
        bms_destroy(sort_);
        bmz_destroy(ctx_);
    }
    gpu_block_compressor(const gpu_block_compressor &) = delete;
    gpu_block_compressor &operator=(const gpu_block_compressor &) = delete;
    void deflate(const uint8_t *in, size_t n, std::vector<uint8_t> &out) override {
        const size_t before = out.size();
        out.resize(before + bmz_bound(n, BMZ_BLOCK_MAX));
        uint64_t got = 0;
        if (bmz_deflate(ctx_, in, n, BMZ_BLOCK_MAX, out.data() + before, out.size() - before, &got) != BMZ_OK)
            throw std::runtime_error(std::string("bmz_deflate: ") + bmz_last_error());
        out.resize(before + got);
    }
    // --sort: the records are put in order on the same device (bms_sort, bms_sort_deflate: the order of include/bms.h, which
    // is the host default's)
    void sort_records(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, std::vector<uint8_t> &sorted,
                      std::vector<uint32_t> &perm, std::vector<uint64_t> &sorted_offset) override {
        sorted.resize(n);
        perm.resize(n_records);
        sorted_offset.resize(n_records + 1);
        if (bms_sort(sorter(), in, n, rec_offset, n_records, sorted.data(), perm.data(), sorted_offset.data()) != BMS_OK)
            throw std::runtime_error(std::string("bms_sort: ") + bms_last_error());
        (void)bms_last_stats(sort_, nullptr, nullptr, nullptr, &passes_);
    }
    void sort_deflate(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, std::vector<uint8_t> &out,
                      std::vector<uint32_t> &perm, std::vector<uint64_t> &sorted_offset) override {
        const size_t before = out.size();
        out.resize(before + bmz_bound(n, BMZ_BLOCK_MAX));
        perm.resize(n_records);
        sorted_offset.resize(n_records + 1);
        uint64_t got = 0;
        if (bms_sort_deflate(sorter(), in, n, rec_offset, n_records, BMZ_BLOCK_MAX, out.data() + before, out.size() - before, &got,
                             perm.data(), sorted_offset.data()) != BMS_OK)
            throw std::runtime_error(std::string("bms_sort_deflate: ") + bms_last_error());
        out.resize(before + got);
        (void)bms_last_stats(sort_, nullptr, nullptr, nullptr, &passes_);
    }
    uint32_t last_sort_passes() const override { return passes_; }
    // --markdup: the descriptors, the marks and the fused mark + sort + deflate on the same device (bmd_*: the rule of
    // include/bmd.h, which is the host default's)
    void dup_ends(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, std::vector<uint64_t> &end,
                  std::vector<uint64_t> &score, std::vector<uint8_t> &kind) override {
        end.resize(n_records);
        score.resize(n_records);
        kind.resize(n_records);
        if (bmd_ends(marker(), in, n, rec_offset, n_records, end.data(), score.data(), kind.data()) != BMD_OK)
            throw std::runtime_error(std::string("bmd_ends: ") + bmd_last_error());
    }
    void dup_mark(const uint64_t *end, const uint64_t *score, const uint8_t *kind, size_t n_records, std::vector<uint8_t> &dup,
                  uint64_t counts[4]) override {
        dup.resize(n_records);
        if (bmd_mark(marker(), end, score, kind, n_records, dup.data(), counts) != BMD_OK)
            throw std::runtime_error(std::string("bmd_mark: ") + bmd_last_error());
    }
    void mark_sort_deflate(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, std::vector<uint8_t> &out,
                           std::vector<uint32_t> &perm, std::vector<uint64_t> &sorted_offset, std::vector<uint8_t> &dup,
                           uint64_t counts[4]) override {
        const size_t before = out.size();
        out.resize(before + bmz_bound(n, BMZ_BLOCK_MAX));
        perm.resize(n_records);
        sorted_offset.resize(n_records + 1);
        dup.resize(n_records);
        uint64_t got = 0;
        if (bmd_mark_sort_deflate(marker(), in, n, rec_offset, n_records, BMZ_BLOCK_MAX, out.data() + before, out.size() - before, &got,
                                  perm.data(), sorted_offset.data(), dup.data(), counts) != BMD_OK)
            throw std::runtime_error(std::string("bmd_mark_sort_deflate: ") + bmd_last_error());
        out.resize(before + got);
        (void)bmd_last_sort_stats(mark_, nullptr, nullptr, nullptr, &passes_);
    }
    // --depth / --coverage: the depth of the written records on the same device (bmc_*: the rule of include/bmc.h, which is
    // the host default's)
    void depth_begin(const uint32_t *ref_len, size_t n_ref) override {
        if (n_ref > 0xFFFFFFFFull) throw std::runtime_error("bmc_begin: " + std::to_string(n_ref) + " references");
        if (bmc_begin(coverer(), ref_len, static_cast<uint32_t>(n_ref)) != BMC_OK) throw std::runtime_error(std::string("bmc_begin: ") + bmc_last_error());
        n_ref_ = n_ref;
    }
    void depth_add(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) override {
        if (bmc_add(coverer(), in, n, rec_offset, n_records, skip) != BMC_OK) throw std::runtime_error(std::string("bmc_add: ") + bmc_last_error());
    }
    void depth_finish(bm::depth_result &out) override {
        uint64_t n_runs = 0;
        out.stats.assign(n_ref_ * bm::kDepthStats, 0);
        if (bmc_finish(coverer(), &n_runs, out.stats.data()) != BMC_OK) throw std::runtime_error(std::string("bmc_finish: ") + bmc_last_error());
        out.runs.assign(static_cast<size_t>(n_runs) * 4, 0);
        if (bmc_runs(cover_, 0, n_runs, out.runs.data()) != BMC_OK) throw std::runtime_error(std::string("bmc_runs: ") + bmc_last_error());
    }
    // --pileup: the allele counts and variant sites of the written records on the same device (bmp_*: the rule of
    // include/bmp.h, which is the host default's)
    void pileup_begin(const uint32_t *ref_len, size_t n_ref, const uint8_t *const *ref_bases, const bm::pileup_thresholds &th) override {
        if (n_ref > 0xFFFFFFFFull) throw std::runtime_error("bmp_begin: " + std::to_string(n_ref) + " references");
        const uint32_t t[BMP_N_THRESHOLDS] = {th.min_mapq, th.min_bq, th.min_alt, th.min_frac_ppm};
        if (bmp_begin(piler(), ref_len, static_cast<uint32_t>(n_ref), ref_bases, t) != BMP_OK)
            throw std::runtime_error(std::string("bmp_begin: ") + bmp_last_error());
        pile_n_ref_ = n_ref;
    }
    void pileup_add(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) override {
        if (bmp_add(piler(), in, n, rec_offset, n_records, skip) != BMP_OK) throw std::runtime_error(std::string("bmp_add: ") + bmp_last_error());
    }
    void pileup_finish(bm::pileup_result &out) override {
        uint64_t n_sites = 0;
        out.stats.assign(pile_n_ref_ * bm::kPileupStats, 0);
        if (bmp_finish(piler(), &n_sites, out.stats.data()) != BMP_OK) throw std::runtime_error(std::string("bmp_finish: ") + bmp_last_error());
        out.sites.assign(static_cast<size_t>(n_sites) * bm::kPileupSiteWords, 0);
        if (bmp_sites(pile_, 0, n_sites, out.sites.data()) != BMP_OK) throw std::runtime_error(std::string("bmp_sites: ") + bmp_last_error());
    }
    // --vcf: the genotypes at the pileup's sites on the same device (bmg_*: the rule of include/bmg.h, which is the host
    // default's)
    void genotype_begin(const uint32_t *ref_len, size_t n_ref, const bm::genotype_params &pr) override {
        if (n_ref > 0xFFFFFFFFull) throw std::runtime_error("bmg_begin: " + std::to_string(n_ref) + " references");
        const uint32_t p[BMG_N_PARAMS] = {pr.min_mapq, pr.min_bq, pr.q_absent, pr.q_cap, pr.prior};
        if (bmg_begin(genotyper(), ref_len, static_cast<uint32_t>(n_ref), p) != BMG_OK) throw std::runtime_error(std::string("bmg_begin: ") + bmg_last_error());
    }
    void genotype_add(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) override {
        if (bmg_add(genotyper(), in, n, rec_offset, n_records, skip) != BMG_OK) throw std::runtime_error(std::string("bmg_add: ") + bmg_last_error());
    }
    void genotype_call(const uint32_t *sites, size_t n_sites, std::vector<uint32_t> &out) override {
        out.assign(n_sites * bm::kGenotypeCallWords, 0);
        if (bmg_call(genotyper(), sites, n_sites, out.data()) != BMG_OK) throw std::runtime_error(std::string("bmg_call: ") + bmg_last_error());
    }
    // --vcf-indels: the indel alleles and calls of the written records on the same device (bmn_*: the rule of include/bmn.h,
    // which is the host default's)
    void indel_begin(const uint32_t *ref_len, size_t n_ref, const bm::indel_params &pr) override {
        if (n_ref > 0xFFFFFFFFull) throw std::runtime_error("bmn_begin: " + std::to_string(n_ref) + " references");
        const uint32_t p[BMN_N_PARAMS] = {pr.min_mapq, pr.min_alt, pr.min_frac_ppm, pr.q_indel, pr.prior};
        if (bmn_begin(indeler(), ref_len, static_cast<uint32_t>(n_ref), p) != BMN_OK) throw std::runtime_error(std::string("bmn_begin: ") + bmn_last_error());
        indel_n_ref_ = n_ref;
    }
    void indel_add(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) override {
        if (bmn_add(indeler(), in, n, rec_offset, n_records, skip) != BMN_OK) throw std::runtime_error(std::string("bmn_add: ") + bmn_last_error());
    }
    void indel_finish(bm::indel_result &out) override {
        uint64_t n_alleles = 0, n_calls = 0;
        out.stats.assign(indel_n_ref_ * bm::kIndelStats, 0);
        if (bmn_finish(indeler(), &out.n_events, &n_alleles, &n_calls, out.stats.data()) != BMN_OK)
            throw std::runtime_error(std::string("bmn_finish: ") + bmn_last_error());
        out.alleles.assign(static_cast<size_t>(n_alleles) * bm::kIndelAlleleWords, 0);
        out.calls.assign(static_cast<size_t>(n_calls) * bm::kIndelCallWords, 0);
        if (bmn_alleles(indel_, 0, n_alleles, out.alleles.data()) != BMN_OK) throw std::runtime_error(std::string("bmn_alleles: ") + bmn_last_error());
        if (bmn_calls(indel_, 0, n_calls, out.calls.data()) != BMN_OK) throw std::runtime_error(std::string("bmn_calls: ") + bmn_last_error());
    }
    // --vcf-bias: strand and MAPQ evidence of the written records and the annotations of the calls on the same device (bmb_*:
    // the rule of include/bmb.h, which is the host default's; the context has uploaded bmb_tables's tables, the argument's)
    void bias_begin(const uint32_t *ref_len, size_t n_ref, const bm::bias_params &pr) override {
        if (n_ref > 0xFFFFFFFFull) throw std::runtime_error("bmb_begin: " + std::to_string(n_ref) + " references");
        const uint32_t p[BMB_N_PARAMS] = {pr.min_mapq, pr.min_bq};
        if (bmb_begin(biaser(), ref_len, static_cast<uint32_t>(n_ref), p) != BMB_OK) throw std::runtime_error(std::string("bmb_begin: ") + bmb_last_error());
    }
    void bias_add(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) override {
        if (bmb_add(biaser(), in, n, rec_offset, n_records, skip) != BMB_OK) throw std::runtime_error(std::string("bmb_add: ") + bmb_last_error());
    }
    void bias_annotate(const uint32_t *calls, size_t n_calls, const bm::bias_tables &, std::vector<uint32_t> &out) override {
        out.assign(n_calls * bm::kBiasOutWords, 0);
        if (bmb_annotate(biaser(), calls, n_calls, out.data()) != BMB_OK) throw std::runtime_error(std::string("bmb_annotate: ") + bmb_last_error());
    }
    // --vcf-phase: the links between the het SNV calls that the written records observe, and the phase from them, on the same
    // device (bmk_*: the rule of include/bmk.h, which is the host default's)
    size_t phase_begin(const uint32_t *ref_len, size_t n_ref, const bm::phase_params &pr, const uint32_t *calls, size_t n_calls) override {
        if (n_ref > 0xFFFFFFFFull) throw std::runtime_error("bmk_begin: " + std::to_string(n_ref) + " references");
        const uint32_t p[BMK_N_PARAMS] = {pr.min_mapq, pr.min_bq, pr.min_links, pr.min_frac_ppm, pr.reach};
        uint64_t n_sites = 0;
        if (bmk_begin(phaser(), ref_len, static_cast<uint32_t>(n_ref), p, calls, n_calls, &n_sites) != BMK_OK)
            throw std::runtime_error(std::string("bmk_begin: ") + bmk_last_error());
        return static_cast<size_t>(n_sites);
    }
    void phase_add(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) override {
        if (bmk_add(phaser(), in, n, rec_offset, n_records, skip) != BMK_OK) throw std::runtime_error(std::string("bmk_add: ") + bmk_last_error());
    }
    void phase_finish(bm::phase_result &out) override {
        uint64_t stats[BMK_N_STATS];
        if (bmk_finish(phaser(), stats) != BMK_OK) throw std::runtime_error(std::string("bmk_finish: ") + bmk_last_error());
        for (size_t k = 0; k < bm::kPhaseStats; k++) out.stats[k] = stats[k];
        out.sites.assign(static_cast<size_t>(stats[BMK_S_SITES]) * bm::kPhaseOutWords, 0);
        if (bmk_phase(phaser(), 0, stats[BMK_S_SITES], out.sites.data()) != BMK_OK) throw std::runtime_error(std::string("bmk_phase: ") + bmk_last_error());
    }
    // --stats: the mapping statistics of the written records on the same device (bmq_*: the rule of include/bmq.h, which is the
    // host default's)
    void stats_begin(const bm::stats_params &pr) override {
        const uint32_t p[BMQ_N_PARAMS] = {pr.max_cycle, pr.max_insert};
        if (bmq_begin(counter(), p) != BMQ_OK) throw std::runtime_error(std::string("bmq_begin: ") + bmq_last_error());
        stats_params_ = pr;
    }
    void stats_add(const uint8_t *in, size_t n, const uint64_t *rec_offset, size_t n_records, const uint8_t *skip) override {
        if (bmq_add(counter(), in, n, rec_offset, n_records, skip) != BMQ_OK) throw std::runtime_error(std::string("bmq_add: ") + bmq_last_error());
    }
    void stats_finish(bm::stats_result &out) override {
        static_assert(BMQ_N_TALLIES == bm::kStatsTallies && BMQ_N_TABLES == bm::kStatsTables, "bmq.h and host/stats.h disagree");
        out = bm::stats_result{};
        out.params = stats_params_;
        if (bmq_finish(counter(), out.tallies) != BMQ_OK) throw std::runtime_error(std::string("bmq_finish: ") + bmq_last_error());
        for (size_t t = 0; t < bm::kStatsTables; t++) {
            const size_t rows = bm::stats_rows(t, stats_params_);
            out.table[t].assign(rows * bm::kStatsWidth[t], 0);
            if (bmq_table(counter(), static_cast<uint32_t>(t), 0, rows, out.table[t].data()) != BMQ_OK)
                throw std::runtime_error(std::string("bmq_table: ") + bmq_last_error());
        }
    }
    // --gvcf: the reference blocks of the genotype caller's cells on the same device (bmr_*: the rule of include/bmr.h, which
    // is the host default's)
    void refblocks(const uint32_t *ref_len, size_t n_ref, const uint8_t *const *ref_bases, const std::vector<uint32_t> &bands,
                   const std::vector<uint32_t> &exclude, bm::refblock_result &out) override {
        if (!blocks_ && bmr_create(device_, &blocks_) != BMR_OK) throw std::runtime_error(std::string("bmr_create: ") + bmr_last_error());
        uint64_t n_blocks = 0;
        if (bmr_run(blocks_, genotyper(), ref_bases, bands.data(), static_cast<uint32_t>(bands.size()), exclude.data(), exclude.size() / 3, &n_blocks) != BMR_OK)
            throw std::runtime_error(std::string("bmr_run: ") + bmr_last_error());
        out.blocks.assign(static_cast<size_t>(n_blocks) * bm::kRefBlockWords, 0);
        if (bmr_blocks(blocks_, 0, n_blocks, out.blocks.data()) != BMR_OK) throw std::runtime_error(std::string("bmr_blocks: ") + bmr_last_error());
        bm::refblock_count_rest(out, std::vector<uint32_t>(ref_len, ref_len + n_ref), exclude);
    }

private:
    int device_ = 0;
    bmr_ctx *blocks_ = nullptr;     // made by the first call: a run without --gvcf pays nothing for it
    bmq_ctx *stats_ = nullptr;      // made by the first stats call: a run without --stats pays nothing for it
    bm::stats_params stats_params_;
    bmq_ctx *counter() {
        if (!stats_ && bmq_create(device_, &stats_) != BMQ_OK) throw std::runtime_error(std::string("bmq_create: ") + bmq_last_error());
        return stats_;
    }
    bmk_ctx *phase_ = nullptr;      // made by the first phase call: a run without --vcf-phase pays nothing for it
    bmk_ctx *phaser() {
        if (!phase_ && bmk_create(device_, &phase_) != BMK_OK) throw std::runtime_error(std::string("bmk_create: ") + bmk_last_error());
        return phase_;
    }
    bmb_ctx *bias_ = nullptr;       // made by the first bias call: a run without --vcf-bias pays nothing for it
    bmb_ctx *biaser() {
        if (!bias_ && bmb_create(device_, &bias_) != BMB_OK) throw std::runtime_error(std::string("bmb_create: ") + bmb_last_error());
        return bias_;
    }
    bmn_ctx *indel_ = nullptr;      // made by the first indel call: a run without --vcf-indels pays nothing for it
    size_t indel_n_ref_ = 0;
    bmn_ctx *indeler() {
        if (!indel_ && bmn_create(device_, &indel_) != BMN_OK) throw std::runtime_error(std::string("bmn_create: ") + bmn_last_error());
        return indel_;
    }
    bmg_ctx *geno_ = nullptr;       // made by the first genotype call: a run without --vcf pays nothing for it
    bmg_ctx *genotyper() {
        if (!geno_ && bmg_create(device_, &geno_) != BMG_OK) throw std::runtime_error(std::string("bmg_create: ") + bmg_last_error());
        return geno_;
    }
    bmp_ctx *pile_ = nullptr;       // made by the first pileup call: a run without --pileup pays nothing for it
    size_t pile_n_ref_ = 0;
    bmp_ctx *piler() {
        if (!pile_ && bmp_create(device_, &pile_) != BMP_OK) throw std::runtime_error(std::string("bmp_create: ") + bmp_last_error());
        return pile_;
    }
    bmc_ctx *cover_ = nullptr;     // made by the first depth call: a run without --depth / --coverage pays nothing for it
    size_t n_ref_ = 0;
    bmc_ctx *coverer() {
        if (!cover_ && bmc_create(device_, &cover_) != BMC_OK) throw std::runtime_error(std::string("bmc_create: ") + bmc_last_error());
        return cover_;
    }
    bmd_ctx *mark_ = nullptr;       // made by the first marking call: a run without --markdup pays nothing for it
    bmd_ctx *marker() {
        if (!mark_ && bmd_create(device_, &mark_) != BMD_OK) throw std::runtime_error(std::string("bmd_create: ") + bmd_last_error());
        return mark_;
    }
    bms_ctx *sort_ = nullptr;       // made by the first sort: a run without --sort pays nothing for it
    uint32_t passes_ = 0;
    bms_ctx *sorter() {
        if (!sort_ && bms_create(device_, &sort_) != BMS_OK) throw std::runtime_error(std::string("bms_create: ") + bms_last_error());
        return sort_;
    }
};
}  // namespace

std::unique_ptr<bm::block_compressor> bm_make_compressor(const bm::cmd_arguments &args) {
    return std::make_unique<gpu_block_compressor>(args.gpus.empty() ? 0 : args.gpus.front());
}

// Compressed -q / --genome: the BGZF blocks are inflated on the first device of --gpus (bmu_inflate).
std::unique_ptr<bm::block_inflater> bm_make_inflater(const bm::cmd_arguments &args) {
    return std::make_unique<bm::gpu_block_inflater>(args.gpus.empty() ? 0 : args.gpus.front());
}

void bm_report_resources(const bm::cmd_arguments &args) {
    struct rusage ru {};
    getrusage(RUSAGE_SELF, &ru);
    std::vector<int> seen;
    for (int dev : args.gpus) {
        if (std::find(seen.begin(), seen.end(), dev) != seen.end()) continue;
        seen.push_back(dev);
        uint64_t free_b = 0, total_b = 0;
        if (bmf_device_memory(dev, &free_b, &total_b) != BMF_OK) continue;
        std::cerr << "[INFO]\t\tDevice " << dev << ": " << static_cast<double>(total_b - free_b) / (1u << 30) << " GiB of "
                  << static_cast<double>(total_b) / (1u << 30) << " GiB in use at the end of the run.\n";
    }
    std::cerr << "[INFO]\t\tHost peak resident set: " << static_cast<double>(ru.ru_maxrss) / (1u << 20) << " GiB.\n";
}
