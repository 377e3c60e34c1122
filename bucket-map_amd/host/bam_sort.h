// bam_sort.h -- coordinate-sorted BAM with a .bai index (-o x.bam --sort): the run buffer, the merge of several runs and the
// index.  The order is that of include/bms.h (bam_sort_key in bgzf.h: refID, then pos + 1, stable); who sorts a run is the
// block_compressor (the device in the product, std::stable_sort elsewhere: the same permutation).
//
// Records are kept, with their offsets, in a run of at most run_bytes of BAM stream (--sort-mem; BM_SORT_RUN_BYTES for the
// tests).  One run: one sort_deflate call at finish().  Several: every full run is sorted (sort_records) and written raw to
// <out>.sort.<k>.tmp; finish() merges the runs by key, ties to the lower run number -- the stable sort of the whole input --
// and deflates the merged stream in pieces of whole blocks.  Blocks are cut by size alone, so both ways give the same bytes.
//
// THE INDEX (SAM spec 5.2), fixed so that the file is a function of the sorted records:
//   - a record at sorted-stream offset so has the virtual offset file_offset(block so / 65280) << 16 | so % 65280; block file
//     offsets are read from the BSIZE fields of the emitted blocks, after the header's blocks; the end of the stream on a
//     block border points at the EOF block;
//   - a record covers [max(pos, 0), pos + reference length of its CIGAR) -- one base if that is empty; for a CG:B,I long CIGAR
//     the placeholder's N carries the length -- and its bin is the record's own bin field;
//   - bins ascending; one chunk per maximal run of consecutive records with the same (refID, bin), from the first record's
//     offset to the offset after the last; no further merging;
//   - linear index in 16 384-base windows: ioffset[w] = the offset of the first record that overlaps w, an untouched window
//     takes the next touched one's value, n_intv = the last touched window + 1;
//   - pseudo-bin 37450 for every reference with a record: (first, end) offsets, then (records without 0x4, records with 0x4);
//   - n_no_coor = the records with refID = -1; a reference without records has n_bin = 0 and n_intv = 0.
//   A record that ends beyond 2^29 cannot be binned by this format: it is refused (CSI is out of scope).
//
// MARK MODE (--markdup; include/bmd.h states the rule, who computes it is again the block_compressor).  Marking needs the
// records in the order they came in, where mates are adjacent, so it happens before the sort.  One run: one mark_sort_deflate
// call at finish(); 0x400 is then ORed into the host copy from the returned marks, because the index's pseudo-bin counts read
// flags and the records it describes must be the written ones.  Several runs: each spill computes the run's descriptors
// (dup_ends) and keeps them and the run's perm -- 17 + 4 bytes per record --, the raw run is sorted and written as before;
// finish() makes one dup_mark over the concatenated descriptors, and the merge ORs 0x400 into record run_base[r] + perm_r[k]
// as it copies the k-th record of run r.  A run never ends between two mates: when the run's last record has 0x1 and 0x40
// (and not 0x80) and the incoming one has 0x80 (and not 0x40), that one is taken into the run first (the run may exceed run_bytes by one record).  Both
// ways give the same files.
//
// DEPTH MODE (--depth / --coverage; include/bmc.h states the rule, who computes it is again the block_compressor).  The records
// counted are the records written, with their final flags, so counting happens in finish(): one run -- the run buffer, after
// the marks have been ORed into it, in one depth_add call; several runs -- the merged stream as it is made, cut at record
// borders into pieces of about run_bytes, one depth_add call each.  The rule does not depend on the order or the cutting of
// the records, so both ways give the same result; it is kept for the caller, who writes the files.
//
// PILEUP MODE (--pileup; include/bmp.h states the rule).  The same pieces of the final stream go to pileup_add, beside or
// without depth mode: pileup_begin with the references' bases and the thresholds before them, pileup_finish after them.
//
// GENOTYPE MODE (--vcf; include/bmg.h states the rule), on top of pileup mode: every piece that goes to pileup_add goes to
// genotype_add too, and after pileup_finish the sites it lists go to genotype_call.
// INDEL MODE (--vcf-indels; include/bmn.h states the rule), on top of genotype mode: every piece that goes to genotype_add
// goes to indel_add too, indel_begin before them and indel_finish after them.
// BLOCK MODE (--gvcf; include/bmr.h states the rule), on top of genotype mode: after genotype_call, and after indel_finish where
// there is one, the positions of the variant calls go to refblocks as excluded intervals.
// BIAS MODE (--vcf-bias; include/bmb.h states the rule), on top of genotype mode: every piece that goes to genotype_add goes to
// bias_add too, and after genotype_call the calls go to bias_annotate.
// PHASE MODE (--vcf-phase; include/bmk.h states the rule), on top of genotype mode: the phase sites are het calls, so the links
// are counted in a SECOND PASS over the final records after genotype_call: phase_begin with the calls, the records to phase_add,
// phase_finish.  The rule does not depend on the order of the records, so nothing is merged: with one run the pass reads the run
// buffer, which is still in memory with the duplicate marks in it; with several it reads each run file in pieces of at most
// run_bytes, ORs the duplicate marks in as the merge does, and the files are removed only after it.
// STATS MODE (--stats; include/bmq.h states the rule), beside or without every other mode: stats_begin before the pieces, every
// piece that goes to depth_add / pileup_add goes to stats_add, stats_finish after them.  The rule needs no reference and does not
// depend on the order or the cutting of the records, so one run and several give the same result.
#pragma once

#include "bgzf.h"

#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <functional>
#include <map>
#include <memory>
#include <ostream>
#include <queue>
#include <stdexcept>
#include <string>
#include <utility>

namespace bm {

// --sort-mem N (MiB) as bytes, unless BM_SORT_RUN_BYTES says otherwise (the tests force several runs on small inputs)
inline size_t bam_sort_run_bytes(size_t mem_mib) {
    if (const char *e = std::getenv("BM_SORT_RUN_BYTES")) {
        const unsigned long long v = std::strtoull(e, nullptr, 10);
        if (v) return static_cast<size_t>(v);
    }
    return mem_mib << 20;
}

class bai_builder {
    static constexpr uint64_t kNone = ~uint64_t{0};
    static constexpr uint32_t kPseudoBin = 37450;
    struct ref_entry {
        std::map<uint32_t, std::vector<std::pair<uint64_t, uint64_t>>> bins;   // stream offsets until write()
        std::vector<uint64_t> linear;
        uint64_t first = 0, end = 0, n_mapped = 0, n_unmapped = 0;
        bool any = false;
    };
    std::vector<ref_entry> refs_;
    uint64_t n_no_coor_ = 0;
    int64_t run_ref_ = -1;                // the open chunk
    uint32_t run_bin_ = 0;
    uint64_t run_beg_ = 0, run_end_ = 0;

    static uint32_t u32(const uint8_t *p) {
        uint32_t v;
        std::memcpy(&v, p, 4);
        return v;
    }
    static uint32_t u16(const uint8_t *p) { return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8; }
    void close_run() {
        if (run_ref_ >= 0) refs_[static_cast<size_t>(run_ref_)].bins[run_bin_].emplace_back(run_beg_, run_end_);
        run_ref_ = -1;
    }

public:
    explicit bai_builder(size_t n_ref) : refs_(n_ref) {}

    // the records in sorted order: rec[0, len) starts at offset so of the sorted stream
    void add(const uint8_t *rec, uint64_t so, uint64_t len) {
        const int32_t ref = static_cast<int32_t>(u32(rec + 4)), pos = static_cast<int32_t>(u32(rec + 8));
        if (ref < 0) {
            close_run();
            n_no_coor_++;
            return;
        }
        if (static_cast<size_t>(ref) >= refs_.size()) throw std::runtime_error("--sort: a record names reference " + std::to_string(ref) + ", the header has " + std::to_string(refs_.size()));
        const uint32_t l_name = rec[12], bin = u16(rec + 14), n_cigar = u16(rec + 16), flag = u16(rec + 18);
        if (36ull + l_name + 4ull * n_cigar > len) throw std::runtime_error("--sort: a record's CIGAR lies beyond its end");
        uint64_t ref_len = 0;
        for (uint32_t k = 0; k < n_cigar; k++) {
            const uint32_t c = u32(rec + 36 + l_name + 4 * k), op = c & 15u;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_len += c >> 4;
        }
        const uint64_t beg = pos < 0 ? 0 : static_cast<uint64_t>(pos);
        const int64_t past = static_cast<int64_t>(pos) + static_cast<int64_t>(ref_len ? ref_len : 1);
        const uint64_t end = past <= static_cast<int64_t>(beg) ? beg + 1 : static_cast<uint64_t>(past);
        if (end > (uint64_t{1} << 29))
            throw std::runtime_error("--sort: a record ends at base " + std::to_string(end) + ", beyond the 2^29 a .bai index can hold");
        ref_entry &e = refs_[static_cast<size_t>(ref)];
        if (run_ref_ == ref && run_bin_ == bin) {
            run_end_ = so + len;
        } else {
            close_run();
            run_ref_ = ref, run_bin_ = bin, run_beg_ = so, run_end_ = so + len;
        }
        const size_t w0 = static_cast<size_t>(beg >> 14), w1 = static_cast<size_t>((end - 1) >> 14);
        if (e.linear.size() <= w1) e.linear.resize(w1 + 1, kNone);
        for (size_t w = w0; w <= w1; w++)
            if (e.linear[w] == kNone) e.linear[w] = so;
        if (!e.any) e.first = so;
        e.any = true;
        e.end = so + len;
        (flag & 4u ? e.n_unmapped : e.n_mapped)++;
    }

    // voffset: sorted-stream offset -> virtual file offset
    void write(std::ostream &out, const std::function<uint64_t(uint64_t)> &voffset) {
        close_run();
        auto p32 = [&](uint32_t v) { out.write(reinterpret_cast<const char *>(&v), 4); };   // little-endian hosts only, as bgzf.h
        auto p64 = [&](uint64_t v) { out.write(reinterpret_cast<const char *>(&v), 8); };
        out.write("BAI\1", 4);
        p32(static_cast<uint32_t>(refs_.size()));
        for (ref_entry &e : refs_) {
            p32(static_cast<uint32_t>(e.bins.size() + (e.any ? 1 : 0)));
            for (const auto &[bin, chunks] : e.bins) {
                p32(bin);
                p32(static_cast<uint32_t>(chunks.size()));
                for (const auto &[a, b] : chunks) p64(voffset(a)), p64(voffset(b));
            }
            if (e.any) {
                p32(kPseudoBin);
                p32(2);
                p64(voffset(e.first)), p64(voffset(e.end));
                p64(e.n_mapped), p64(e.n_unmapped);
            }
            p32(static_cast<uint32_t>(e.linear.size()));
            uint64_t next = kNone;
            for (size_t w = e.linear.size(); w-- > 0;) {
                if (e.linear[w] == kNone) e.linear[w] = next;
                next = e.linear[w];
            }
            for (uint64_t so : e.linear) p64(voffset(so));
        }
        p64(n_no_coor_);
    }
};

class bam_sorter {
    block_compressor *z_;
    std::string out_path_;
    size_t run_bytes_;
    std::vector<uint8_t> run_;
    std::vector<uint64_t> off_{0};
    std::vector<std::string> tmp_;
    uint64_t n_records_ = 0;
    uint32_t passes_ = 0;
    bool mark_ = false;                              // mark mode
    std::vector<uint64_t> desc_end_, desc_score_;    // several runs: the descriptors of all runs so far, in input order
    std::vector<uint8_t> desc_kind_;
    std::vector<std::vector<uint32_t>> run_perm_;    // ... and each run's perm
    uint64_t counts_[4] = {0, 0, 0, 0};
    bool depth_ = false;                             // depth mode
    std::vector<uint32_t> depth_ref_len_;
    depth_result depth_result_;
    bool pileup_ = false;                            // pileup mode
    std::vector<uint32_t> pileup_ref_len_;
    std::vector<const uint8_t *> pileup_ref_bases_;
    pileup_thresholds pileup_thresholds_;
    pileup_result pileup_result_;
    bool genotype_ = false;                          // genotype mode (with pileup mode)
    genotype_params genotype_params_;
    genotype_result genotype_result_;
    bool indel_ = false;                             // indel mode (with genotype mode)
    indel_params indel_params_;
    indel_result indel_result_;
    bool refblocks_ = false;                         // block mode (with genotype mode)
    std::vector<uint32_t> refblock_bands_;
    refblock_result refblock_result_;
    bool bias_ = false;                              // bias mode (with genotype mode)
    bias_params bias_params_;
    const bias_tables *bias_tables_ = nullptr;
    std::vector<uint32_t> bias_notes_;
    bool phase_ = false;                             // phase mode (with genotype mode)
    phase_params phase_params_;
    phase_result phase_result_;
    bool stats_ = false;                             // stats mode
    stats_params stats_params_;
    stats_result stats_result_;

    static uint32_t u32(const uint8_t *p) {
        uint32_t v;
        std::memcpy(&v, p, 4);
        return v;
    }
    void remove_tmp() noexcept {
        for (const std::string &t : tmp_) std::remove(t.c_str());
        tmp_.clear();
    }
    // the run, sorted, as a raw file of its own
    void spill() {
        std::vector<uint8_t> sorted;
        std::vector<uint32_t> perm;
        std::vector<uint64_t> so;
        if (mark_) {
            std::vector<uint64_t> end, score;
            std::vector<uint8_t> kind;
            z_->dup_ends(run_.data(), run_.size(), off_.data(), off_.size() - 1, end, score, kind);
            desc_end_.insert(desc_end_.end(), end.begin(), end.end());
            desc_score_.insert(desc_score_.end(), score.begin(), score.end());
            desc_kind_.insert(desc_kind_.end(), kind.begin(), kind.end());
        }
        z_->sort_records(run_.data(), run_.size(), off_.data(), off_.size() - 1, sorted, perm, so);
        passes_ = std::max(passes_, z_->last_sort_passes());
        if (mark_) run_perm_.push_back(perm);
        tmp_.push_back(out_path_ + ".sort." + std::to_string(tmp_.size()) + ".tmp");   // listed first: removed whatever happens next
        std::ofstream f(tmp_.back(), std::ios::binary);
        f.write(reinterpret_cast<const char *>(sorted.data()), static_cast<std::streamsize>(sorted.size()));
        f.close();
        if (!f) throw std::runtime_error("--sort: cannot write " + tmp_.back());
        run_.clear();
        off_.assign(1, 0);
    }

    struct run_reader {
        std::ifstream f;
        std::vector<uint8_t> rec;
        bool next() {
            uint8_t head[4];
            if (!f.read(reinterpret_cast<char *>(head), 4)) return false;
            const uint32_t size = u32(head);
            rec.resize(4 + static_cast<size_t>(size));
            std::memcpy(rec.data(), head, 4);
            if (!f.read(reinterpret_cast<char *>(rec.data()) + 4, size)) throw std::runtime_error("--sort: a run file ends inside a record");
            return true;
        }
    };

public:
    bam_sorter(block_compressor *z, const std::filesystem::path &out_path, size_t run_bytes, bool mark = false)
        : z_(z), out_path_(out_path.string()), run_bytes_(std::max<size_t>(run_bytes, 1)), mark_(mark) {}
    ~bam_sorter() { remove_tmp(); }
    bam_sorter(const bam_sorter &) = delete;
    bam_sorter &operator=(const bam_sorter &) = delete;

    uint64_t n_records() const { return n_records_; }
    size_t n_runs() const { return n_runs_; }
    uint32_t n_passes() const { return passes_; }
    // mark mode, after finish(): pair units, fragment units, duplicate records from pair units, duplicate fragment records
    const uint64_t *dup_counts() const { return counts_; }
    // depth mode: before the first add(), the references' lengths; after finish(), the runs and the sums per reference
    void set_depth(const std::vector<size_t> &ref_lengths) {
        depth_ = true;
        depth_ref_len_.clear();
        for (size_t len : ref_lengths) {
            if (len > 0xFFFFFFFFull) throw std::runtime_error("--depth: a reference of " + std::to_string(len) + " bases");
            depth_ref_len_.push_back(static_cast<uint32_t>(len));
        }
    }
    const depth_result &depth() const { return depth_result_; }
    // pileup mode: before the first add(), the references' lengths, their bases (ref_bases[r]: ref_lengths[r] bytes that stay
    // where they are until finish() is done) and the thresholds; after finish(), the sites and the sums per reference
    void set_pileup(const std::vector<size_t> &ref_lengths, const std::vector<const uint8_t *> &ref_bases, const pileup_thresholds &th) {
        pileup_ = true;
        pileup_ref_len_.clear();
        for (size_t len : ref_lengths) {
            if (len > 0xFFFFFFFFull) throw std::runtime_error("--pileup: a reference of " + std::to_string(len) + " bases");
            pileup_ref_len_.push_back(static_cast<uint32_t>(len));
        }
        pileup_ref_bases_ = ref_bases;
        pileup_thresholds_ = th;
    }
    const pileup_result &pileup() const { return pileup_result_; }
    // genotype mode: after set_pileup (whose references and sites it uses) and before the first add(); after finish(), one call
    // per site of the pileup
    void set_genotype(const genotype_params &pr) {
        if (!pileup_) throw std::runtime_error("--vcf: genotypes are called at the sites of the pileup");
        genotype_ = true;
        genotype_params_ = pr;
    }
    const genotype_result &genotype() const { return genotype_result_; }
    // indel mode: after set_genotype and before the first add(); after finish(), the alleles and calls of the indels
    void set_indel(const indel_params &pr) {
        if (!genotype_) throw std::runtime_error("--vcf-indels: the indel calls go into the file of --vcf");
        indel_ = true;
        indel_params_ = pr;
    }
    const indel_result &indel() const { return indel_result_; }
    // block mode: after set_genotype and before the first add(); after finish(), the reference blocks between the variant calls
    void set_refblocks(const std::vector<uint32_t> &bands) {
        if (!genotype_) throw std::runtime_error("--gvcf: the blocks are made of the genotype caller's cells");
        refblocks_ = true;
        refblock_bands_ = bands;
    }
    const refblock_result &refblocks() const { return refblock_result_; }
    // bias mode: after set_genotype and before the first add(); after finish(), one annotation per call of the genotype
    // caller.  The tables are bmb_tables's and outlive the sorter.
    void set_bias(const bias_params &pr, const bias_tables &tables) {
        if (!genotype_) throw std::runtime_error("--vcf-bias: the annotations belong to the calls of --vcf");
        bias_ = true;
        bias_params_ = pr;
        bias_tables_ = &tables;
    }
    const std::vector<uint32_t> &bias_notes() const { return bias_notes_; }
    // phase mode: after set_genotype and before the first add(); after finish(), eight words per het SNV call and the sums
    void set_phase(const phase_params &pr) {
        if (!genotype_) throw std::runtime_error("--vcf-phase: the phase belongs to the calls of --vcf");
        phase_ = true;
        phase_params_ = pr;
    }
    const phase_result &phase() const { return phase_result_; }
    // stats mode: before the first add(); after finish(), the tallies and tables of the records written
    void set_stats(const stats_params &pr) {
        stats_ = true;
        stats_params_ = pr;
    }
    const stats_result &stats() const { return stats_result_; }

    // whole records, back to back
    void add(const uint8_t *recs, size_t n) {
        for (size_t at = 0; at < n;) {
            if (n - at < 4) throw std::runtime_error("--sort: a truncated record");
            const size_t len = 4 + static_cast<size_t>(u32(recs + at));
            if (len < 36 || len > n - at) throw std::runtime_error("--sort: a record of " + std::to_string(len) + " bytes");
            if (off_.size() > 1 && (run_.size() + len > run_bytes_ || off_.size() > 0x7FFFFFFFu - (mark_ ? 1u : 0u))) {
                // mark mode: no run ends between two mates
                const uint8_t *last = run_.data() + off_[off_.size() - 2];
                const bool keep = mark_ && (last[18] & 0xC1u) == 0x41u && (recs[at + 18] & 0xC0u) == 0x80u && off_.size() <= 0x7FFFFFFFu;
                if (!keep) spill();
            }
            run_.insert(run_.end(), recs + at, recs + at + len);
            off_.push_back(run_.size());
            n_records_++;
            at += len;
        }
    }

    // the sorted records as BGZF blocks and the EOF block to `out` (which holds header_bytes of header blocks already), the
    // index to <out path>.bai
    void finish(std::ostream &out, uint64_t header_bytes, size_t n_ref) {
        bai_builder bai(n_ref);
        std::vector<uint64_t> block_at{header_bytes};
        std::vector<uint8_t> blocks;
        auto emit = [&]() {                              // the blocks made so far: to the file, their offsets noted
            for (size_t at = 0; at < blocks.size();) {
                const size_t size = (static_cast<size_t>(blocks[at + 16]) | static_cast<size_t>(blocks[at + 17]) << 8) + 1;
                block_at.push_back(block_at.back() + size);
                at += size;
            }
            out.write(reinterpret_cast<const char *>(blocks.data()), static_cast<std::streamsize>(blocks.size()));
            blocks.clear();
        };
        if (depth_) z_->depth_begin(depth_ref_len_.data(), depth_ref_len_.size());
        if (pileup_) z_->pileup_begin(pileup_ref_len_.data(), pileup_ref_len_.size(), pileup_ref_bases_.data(), pileup_thresholds_);
        if (genotype_) z_->genotype_begin(pileup_ref_len_.data(), pileup_ref_len_.size(), genotype_params_);
        if (indel_) z_->indel_begin(pileup_ref_len_.data(), pileup_ref_len_.size(), indel_params_);
        if (bias_) z_->bias_begin(pileup_ref_len_.data(), pileup_ref_len_.size(), bias_params_);
        if (stats_) z_->stats_begin(stats_params_);
        std::vector<uint8_t> dup;                        // mark mode, several runs: one marking over all runs' descriptors;
        std::vector<uint64_t> run_base;                  // run r's records are dup[run_base[r] ..] in input order (the phase pass reads both again)
        if (tmp_.empty()) {
            n_runs_ = off_.size() > 1 ? 1 : 0;
            std::vector<uint32_t> perm;
            std::vector<uint64_t> so;
            if (mark_) {
                std::vector<uint8_t> dup;
                z_->mark_sort_deflate(run_.data(), run_.size(), off_.data(), off_.size() - 1, blocks, perm, so, dup, counts_);
                for (size_t i = 0; i + 1 < off_.size(); i++)
                    if (dup[i]) run_[off_[i] + 19] |= 4;
            } else {
                z_->sort_deflate(run_.data(), run_.size(), off_.data(), off_.size() - 1, blocks, perm, so);
            }
            passes_ = z_->last_sort_passes();
            for (size_t k = 0; k + 1 < off_.size(); k++) bai.add(run_.data() + off_[perm[k]], so[k], so[k + 1] - so[k]);
            emit();
            if (depth_) z_->depth_add(run_.data(), run_.size(), off_.data(), off_.size() - 1, nullptr);
            if (pileup_) z_->pileup_add(run_.data(), run_.size(), off_.data(), off_.size() - 1, nullptr);
            if (genotype_) z_->genotype_add(run_.data(), run_.size(), off_.data(), off_.size() - 1, nullptr);
            if (indel_) z_->indel_add(run_.data(), run_.size(), off_.data(), off_.size() - 1, nullptr);
            if (bias_) z_->bias_add(run_.data(), run_.size(), off_.data(), off_.size() - 1, nullptr);
            if (stats_) z_->stats_add(run_.data(), run_.size(), off_.data(), off_.size() - 1, nullptr);
        } else {
            if (off_.size() > 1) spill();
            n_runs_ = tmp_.size();
            std::vector<uint8_t>().swap(run_);
            std::vector<uint64_t> taken(tmp_.size(), 0);
            run_base.assign(tmp_.size() + 1, 0);
            if (mark_) {
                z_->dup_mark(desc_end_.data(), desc_score_.data(), desc_kind_.data(), desc_kind_.size(), dup, counts_);
                for (size_t r = 0; r < tmp_.size(); r++) run_base[r + 1] = run_base[r] + run_perm_[r].size();
            }
            std::vector<std::unique_ptr<run_reader>> reader;
            using item = std::pair<uint64_t, size_t>;    // (key, run): the lower run wins a tie, and a run is in order already
            std::priority_queue<item, std::vector<item>, std::greater<item>> heap;
            for (size_t r = 0; r < tmp_.size(); r++) {
                reader.push_back(std::make_unique<run_reader>());
                reader[r]->f.open(tmp_[r], std::ios::binary);
                if (!reader[r]->f) throw std::runtime_error("--sort: cannot read " + tmp_[r]);
                if (reader[r]->next()) heap.emplace(bam_sort_key(reader[r]->rec.data()), r);
            }
            constexpr size_t kPiece = size_t{64} * kBgzfBlockMax;
            std::vector<uint8_t> merged, counted;        // counted: depth, pileup or stats mode, the merged records not yet handed to depth_add / pileup_add
            std::vector<uint64_t> counted_off{0};
            auto count = [&]() {
                if (depth_ && counted_off.size() > 1) z_->depth_add(counted.data(), counted.size(), counted_off.data(), counted_off.size() - 1, nullptr);
                if (pileup_ && counted_off.size() > 1) z_->pileup_add(counted.data(), counted.size(), counted_off.data(), counted_off.size() - 1, nullptr);
                if (genotype_ && counted_off.size() > 1) z_->genotype_add(counted.data(), counted.size(), counted_off.data(), counted_off.size() - 1, nullptr);
                if (indel_ && counted_off.size() > 1) z_->indel_add(counted.data(), counted.size(), counted_off.data(), counted_off.size() - 1, nullptr);
                if (bias_ && counted_off.size() > 1) z_->bias_add(counted.data(), counted.size(), counted_off.data(), counted_off.size() - 1, nullptr);
                if (stats_ && counted_off.size() > 1) z_->stats_add(counted.data(), counted.size(), counted_off.data(), counted_off.size() - 1, nullptr);
                counted.clear();
                counted_off.assign(1, 0);
            };
            uint64_t so = 0;
            while (!heap.empty()) {
                const size_t r = heap.top().second;
                heap.pop();
                std::vector<uint8_t> &rec = reader[r]->rec;
                if (mark_ && dup[run_base[r] + run_perm_[r][taken[r]++]]) rec[19] |= 4;
                bai.add(rec.data(), so, rec.size());
                so += rec.size();
                merged.insert(merged.end(), rec.begin(), rec.end());
                if (depth_ || pileup_ || stats_) {
                    counted.insert(counted.end(), rec.begin(), rec.end());
                    counted_off.push_back(counted.size());
                    if (counted.size() >= run_bytes_) count();
                }
                if (merged.size() >= kPiece) {
                    const size_t take = merged.size() / kBgzfBlockMax * kBgzfBlockMax;
                    z_->deflate(merged.data(), take, blocks);
                    emit();
                    merged.erase(merged.begin(), merged.begin() + static_cast<std::ptrdiff_t>(take));
                }
                if (reader[r]->next()) heap.emplace(bam_sort_key(reader[r]->rec.data()), r);
            }
            if (!merged.empty()) z_->deflate(merged.data(), merged.size(), blocks);
            emit();
            if (depth_ || pileup_ || stats_) count();
            reader.clear();
        }
        out.write(reinterpret_cast<const char *>(kBgzfEof), sizeof kBgzfEof);
        if (!out) throw std::runtime_error("--sort: writing " + out_path_ + " failed");
        std::ofstream index(out_path_ + ".bai", std::ios::binary);
        bai.write(index, [&](uint64_t so) { return block_at[static_cast<size_t>(so / kBgzfBlockMax)] << 16 | so % kBgzfBlockMax; });
        index.close();
        if (!index) throw std::runtime_error("--sort: cannot write " + out_path_ + ".bai");
        if (!phase_) remove_tmp();                       // phase mode reads the run files once more
        if (depth_) z_->depth_finish(depth_result_);
        if (pileup_) z_->pileup_finish(pileup_result_);
        if (stats_) z_->stats_finish(stats_result_);
        if (genotype_) {
            z_->genotype_call(pileup_result_.sites.data(), pileup_result_.n_sites(), genotype_result_.calls);
            genotype_result_.n_snv_sites = 0;
            for (size_t k = 0; k < pileup_result_.n_sites(); k++) genotype_result_.n_snv_sites += pileup_result_.sites[kPileupSiteWords * k + 11] & 1u;
        }
        if (bias_) z_->bias_annotate(genotype_result_.calls.data(), genotype_result_.n_calls(), *bias_tables_, bias_notes_);
        if (phase_) {
            phase_pass(dup, run_base);
            remove_tmp();
        }
        if (indel_) z_->indel_finish(indel_result_);
        if (refblocks_)
            z_->refblocks(pileup_ref_len_.data(), pileup_ref_len_.size(), pileup_ref_bases_.data(), refblock_bands_,
                          refblock_excluded(genotype_result_, indel_ ? &indel_result_.calls : nullptr, pileup_ref_len_), refblock_result_);
    }

private:
    size_t n_runs_ = 0;

    // phase mode, after genotype_call: the final records once more, in any order.  One run: run_, as add() filled it and
    // finish() marked it.  Several: each run file in pieces of at most run_bytes_ (a longer record is a piece of its own), the
    // k-th record of file r marked from dup[run_base[r] + run_perm_[r][k]] as the merge marks it.
    void phase_pass(const std::vector<uint8_t> &dup, const std::vector<uint64_t> &run_base) {
        z_->phase_begin(pileup_ref_len_.data(), pileup_ref_len_.size(), phase_params_, genotype_result_.calls.data(), genotype_result_.n_calls());
        if (tmp_.empty()) {
            if (off_.size() > 1) z_->phase_add(run_.data(), run_.size(), off_.data(), off_.size() - 1, nullptr);
        } else {
            std::vector<uint8_t> piece;
            std::vector<uint64_t> piece_off{0};
            auto hand_over = [&]() {
                if (piece_off.size() > 1) z_->phase_add(piece.data(), piece.size(), piece_off.data(), piece_off.size() - 1, nullptr);
                piece.clear();
                piece_off.assign(1, 0);
            };
            for (size_t r = 0; r < tmp_.size(); r++) {
                run_reader reader;
                reader.f.open(tmp_[r], std::ios::binary);
                if (!reader.f) throw std::runtime_error("--sort: cannot read " + tmp_[r]);
                for (uint64_t k = 0; reader.next(); k++) {
                    if (mark_ && dup[run_base[r] + run_perm_[r][k]]) reader.rec[19] |= 4;
                    if (piece_off.size() > 1 && piece.size() + reader.rec.size() > run_bytes_) hand_over();
                    piece.insert(piece.end(), reader.rec.begin(), reader.rec.end());
                    piece_off.push_back(piece.size());
                }
                hand_over();
            }
        }
        z_->phase_finish(phase_result_);
    }
};

}  // namespace bm
