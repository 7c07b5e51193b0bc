// sfgpu_sailfish.hpp -- the C++ host side above the C ABI: drop-in counterparts of the reference classes that sit on
// the quantification hot path, with the reference's names, argument meaning and error behaviour, so that host code
// written against the reference (src/SailfishQuantify.cpp) compiles against these instead.
//
//   sailfish::gpu::TranscriptGroup / TGValue      include/TranscriptGroup.hpp:9-35, EquivalenceClassBuilder.hpp:5-38
//   sailfish::gpu::EquivalenceClassBuilder        include/EquivalenceClassBuilder.hpp:40-119
//   sailfish::gpu::Transcript                     include/Transcript.hpp:14-99, 204-206 (the members the path touches)
//   sailfish::gpu::SailfishOpts                   include/SailfishOpts.hpp:9-41 (the members the path reads)
//   sailfish::gpu::ReadExperiment                 include/ReadExperiment.hpp:65-99, 236-257
//   sailfish::gpu::CollapsedEMOptimizer           include/CollapsedEMOptimizer.hpp:20-35, src/CollapsedEMOptimizer.cpp:557-893
//   sailfish::gpu::CollapsedGibbsSampler          include/CollapsedGibbsSampler.hpp:22-32, src/CollapsedGibbsSampler.cpp:187-291
//   sailfish::gpu::loadEquivClasses               src/SailfishQuantify.cpp:1444-1494 (commented out there; --readEqClasses :1114)
//   sailfish::gpu::writeEquivCounts               src/GZipWriter.cpp:51-92 (the class lines are formatted on the device)
//   sailfish::gpu::writeBootstraps                src/GZipWriter.cpp:249-285 (bootstraps.gz compressed on the device)
//   sailfish::gpu::writeAbundances                src/GZipWriter.cpp:194-248 (the rows of quant.sf are formatted on the device)
//   sailfish::gpu::aggregateEstimatesToGeneLevel  src/SailfishUtils.cpp:929-1037 (genes folded and formatted on the device)
//   sailfish::gpu::readTranscriptToGeneMap        src/SailfishUtils.cpp:322-507 (the --geneMap file read, sorted and joined on the device)
//
// Header only; needs sfgpu.h, the HIP runtime API (hipMalloc / hipMemcpy for the caller-owned buffers the ABI takes)
// and C++14.  No Boost, TBB, spdlog or Eigen: the logger is a std::function<void(int level, const std::string&)>.
// Compiled and run by tests/test_abi.py (tests/cpp_host_test.cpp).
#ifndef SFGPU_SAILFISH_HPP
#define SFGPU_SAILFISH_HPP

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdint>
#include <fstream>
#include <iterator>
#include <functional>
#include <memory>
#include <mutex>
#include <random>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>

#include "sfgpu.h"

namespace sailfish {
namespace gpu {

using Logger = std::function<void(int, const std::string&)>;     // level 0 info, 1 warn, 2 error (spdlog's jointLog)

inline void check_hip(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
inline void check(int rc, const char* what) {
    if (rc != SFGPU_OK) throw std::runtime_error(std::string(what) + ": " + sfgpu_last_error());
}

// caller-owned device buffer (the ABI never allocates what it hands back)
template <typename T>
class DeviceBuf {
  public:
    DeviceBuf() = default;
    explicit DeviceBuf(size_t n) { resize(n); }
    explicit DeviceBuf(const std::vector<T>& h) { resize(h.size()); upload(h); }
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    ~DeviceBuf() { if (p_) (void)hipFree(p_); }
    void resize(size_t n) {
        if (p_) { (void)hipFree(p_); p_ = nullptr; }
        n_ = n;
        check_hip(hipMalloc(reinterpret_cast<void**>(&p_), (n ? n : 1) * sizeof(T)), "hipMalloc");
    }
    void upload(const std::vector<T>& h) { if (n_) check_hip(hipMemcpy(p_, h.data(), n_ * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy"); }
    std::vector<T> download() const {
        std::vector<T> h(n_);
        if (n_) check_hip(hipMemcpy(h.data(), p_, n_ * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy");
        return h;
    }
    T* get() const { return p_; }
    size_t size() const { return n_; }
  private:
    T* p_ = nullptr; size_t n_ = 0;
};

// ---- include/TranscriptGroup.hpp:9-35 --------------------------------------------------------------------
class TranscriptGroup {
  public:
    TranscriptGroup() = default;
    explicit TranscriptGroup(std::vector<uint32_t> txpsIn) : txps(std::move(txpsIn)) {}
    TranscriptGroup(std::vector<uint32_t> txpsIn, size_t hashIn) : txps(std::move(txpsIn)), hash(hashIn) {}
    std::vector<uint32_t> txps;
    size_t hash = 0;            // XXH64 of the id bytes, seed 0 (src/TranscriptGroup.cpp:9-12): filled by eqVec()
    double totalMass = 0.0;
    mutable bool valid = true;
};
inline bool operator==(const TranscriptGroup& a, const TranscriptGroup& b) { return a.txps == b.txps; }

// EquivalenceClassBuilder.hpp:5-38.  The weights are 1.0 at every addGroup call site and optimize() overwrites them;
// eqVec() returns them as optimize() would first set them only on request (they are not stored on the device).
struct TGValue {
    TGValue() = default;
    TGValue(std::vector<double> w, uint64_t c) : weights(std::move(w)), count(c) {}
    mutable std::vector<double> weights;
    uint64_t count = 0;
};

// ---- include/EquivalenceClassBuilder.hpp:40-119 ----------------------------------------------------------
class EquivalenceClassBuilder {
  public:
    explicit EquivalenceClassBuilder(Logger loggerIn = nullptr) : logger_(std::move(loggerIn)) {
        check(sfgpu_eq_create(&h_, 1000000 /* countMap_.reserve(1000000), :44 */, nullptr), "sfgpu_eq_create");
    }
    ~EquivalenceClassBuilder() { if (h_) sfgpu_eq_destroy(h_); }
    EquivalenceClassBuilder(const EquivalenceClassBuilder&) = delete;
    EquivalenceClassBuilder& operator=(const EquivalenceClassBuilder&) = delete;

    void start() { check(sfgpu_eq_start(h_), "sfgpu_eq_start"); active_ = true; vec_.clear(); }        // :62

    // :90-108, called concurrently by the mapping threads; a thread's reads travel in batches of at most 1000
    // (the reference's parser job size, src/SailfishQuantify.cpp:73).  `weights` are all 1.0 and are dropped.
    inline void addGroup(TranscriptGroup&& g, std::vector<double>& /*weights*/) {
        Batch& b = my_batch();
        b.ids.insert(b.ids.end(), g.txps.begin(), g.txps.end());
        b.offsets.push_back(static_cast<uint32_t>(b.ids.size()));
        if (b.offsets.size() > 1000) flush(b);
    }

    // :82-88  single-threaded bulk insert of a known group with a count
    inline void insertGroup(TranscriptGroup g, uint32_t count) {
        pending_ids_.insert(pending_ids_.end(), g.txps.begin(), g.txps.end());
        pending_off_.push_back(static_cast<uint32_t>(pending_ids_.size()));
        pending_cnt_.push_back(count);
    }

    // :64-80  every mapping thread has joined by now (src/SailfishQuantify.cpp:941): their last partial batches go in
    bool finish() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (auto& b : batches_) flush(*b);
        }
        if (!pending_cnt_.empty()) {
            DeviceBuf<uint32_t> ids(pending_ids_), off(pending_off_); DeviceBuf<uint64_t> cnt(pending_cnt_);
            check(sfgpu_eq_add_weighted_device(h_, ids.get(), off.get(), cnt.get(), static_cast<uint32_t>(pending_cnt_.size())),
                  "sfgpu_eq_add_weighted_device");
            pending_ids_.clear(); pending_off_.assign(1, 0); pending_cnt_.clear();
        }
        check(sfgpu_eq_finish(h_, &n_classes_, &nnz_, &total_reads_), "sfgpu_eq_finish");
        active_ = false;
        return true;
    }

    // :110-112  the classes on the host, canonical order (first id, hash, length, label) -- the reference's order is
    // the cuckoo table's and changes from run to run.  For hosts that want the vector: optimize() and writeEquivCounts (below)
    // work from the device table.
    std::vector<std::pair<const TranscriptGroup, TGValue>>& eqVec() {
        if (vec_.empty() && n_classes_) {
            std::vector<uint32_t> rowptr(n_classes_ + 1), ids(nnz_ ? nnz_ : 1);
            std::vector<uint64_t> counts(n_classes_), hashes(n_classes_);
            check(sfgpu_eq_export_host(h_, rowptr.data(), ids.data(), counts.data(), hashes.data()), "sfgpu_eq_export_host");
            vec_.reserve(n_classes_);
            for (uint64_t c = 0; c < n_classes_; ++c) {
                std::vector<uint32_t> lab(ids.begin() + rowptr[c], ids.begin() + rowptr[c + 1]);
                const size_t k = lab.size();
                vec_.emplace_back(TranscriptGroup(std::move(lab), static_cast<size_t>(hashes[c])), TGValue(std::vector<double>(k, 1.0), counts[c]));
            }
        }
        return vec_;
    }

    uint64_t numClasses() const { return n_classes_; }
    uint64_t numNonzeros() const { return nnz_; }
    uint64_t totalReads() const { return total_reads_; }       // what finish() logs as "Counted ... total reads" (:77-78)
    sfgpu_eq* handle() const { return h_; }

  private:
    struct Batch { std::vector<uint32_t> ids; std::vector<uint32_t> offsets{0}; };
    static uint64_t next_id() { static std::atomic<uint64_t> n{1}; return n.fetch_add(1); }
    Batch& my_batch() {
        thread_local std::vector<std::pair<uint64_t, Batch*>> mine;       // keyed by a never-reused builder id
        for (auto& e : mine) if (e.first == id_) return *e.second;
        std::lock_guard<std::mutex> lk(mu_);
        batches_.emplace_back(new Batch());
        mine.emplace_back(id_, batches_.back().get());
        return *batches_.back();
    }
    void flush(Batch& b) {
        const uint32_t n = static_cast<uint32_t>(b.offsets.size() - 1);
        if (n) check(sfgpu_eq_add_batch_host(h_, b.ids.empty() ? &zero_ : b.ids.data(), b.offsets.data(), n), "sfgpu_eq_add_batch_host");
        b.ids.clear(); b.offsets.assign(1, 0);
    }
    sfgpu_eq* h_ = nullptr;
    const uint64_t id_ = next_id();
    Logger logger_;
    bool active_ = false;
    std::mutex mu_;
    std::vector<std::unique_ptr<Batch>> batches_;
    std::vector<uint32_t> pending_ids_, pending_off_{0}; std::vector<uint64_t> pending_cnt_;
    uint64_t n_classes_ = 0, nnz_ = 0, total_reads_ = 0;
    std::vector<std::pair<const TranscriptGroup, TGValue>> vec_;
    uint32_t zero_ = 0;
};

// ---- include/Transcript.hpp (the members the path reads and writes) ---------------------------------------
class Transcript {
  public:
    Transcript(size_t idIn, const char* name, uint32_t len) : RefName(name), RefLength(len), EffectiveLength(-1.0), id(static_cast<uint32_t>(idIn)) {}
    void setEstCount(double sc) { estCount_ = sc; }
    double estCount() const { return estCount_; }
    void setMass(double m) { mass_ = m; }
    double mass() const { return mass_; }
    void setActive() { active_ = true; }
    bool getActive() const { return active_; }
    std::string RefName;
    uint32_t RefLength;
    double EffectiveLength;
    uint32_t id;
  private:
    double mass_ = 0.0, estCount_ = 0.0;
    bool active_ = false;
};

// ---- include/SailfishOpts.hpp:9-41 (the members the path consults) ----------------------------------------
struct SailfishOpts {
    uint32_t numThreads = 1;
    bool useVBOpt = false;
    bool noEffectiveLengthCorrection = false;
    uint32_t numBootstraps = 0;
    uint32_t numGibbsSamples = 0;
    bool biasCorrect = false, gcBiasCorrect = false;
    uint32_t gcSampFactor = 1;      // --gcSizeSamp
    uint32_t pdfSampFactor = 1;     // --gcSpeedSamp
    Logger jointLog;
};

// ---- include/ReadExperiment.hpp:65-99, 236-257 ------------------------------------------------------------
class ReadExperiment {
  public:
    explicit ReadExperiment(Logger log = nullptr) : eqBuilder_(std::move(log)) {}
    std::vector<Transcript>& transcripts() { return transcripts_; }
    EquivalenceClassBuilder& equivalenceClassBuilder() { return eqBuilder_; }
    uint64_t numMappedFragments() const { return numMappedFragments_.load(); }
    std::atomic<uint64_t>& numMappedFragmentsAtomic() { return numMappedFragments_; }
    std::atomic<uint64_t>& numObservedFragmentsAtomic() { return numObservedFragments_; }
    double mappingRate() const {
        const double obs = static_cast<double>(numObservedFragments_.load());
        return obs > 0.0 ? static_cast<double>(numMappedFragments_.load()) / obs : 0.0;
    }
    // what bias correction reads and writes (:93-97, 160-212, 240-255)
    void setSequences(std::string seq, std::vector<uint64_t> txpOffsets) { seq_ = std::move(seq); seqOff_ = std::move(txpOffsets); }   // RapMapSAIndex::seq / txpOffsets (:108-117)
    const std::string& sequences() const { return seq_; }
    const std::vector<uint64_t>& sequenceOffsets() const { return seqOff_; }
    void setFragLengthDist(const std::vector<int32_t>& fldIn) { fld_.assign(fldIn.begin(), fldIn.end()); }
    const std::vector<uint32_t>& fragLengthCounts() const { return fld_; }
    std::vector<uint32_t>& readBias() { return readBias_; }                      // ReadKmerDist<6>::counts, pseudo-count 1
    std::vector<uint32_t>& observedGC() { return observedGC_; }                  // 101 bins, pseudo-count 1
    std::vector<double>& expectedSeqBias() { return expectedSeqBias_; }
    std::vector<double>& expectedGCBias() { return expectedGC_; }
    void addNumFwd(int32_t n) { numFwd_ += n; }
    void addNumRC(int32_t n) { numRC_ += n; }
    int64_t numFwd() const { return numFwd_.load(); }
    int64_t numRC() const { return numRC_.load(); }
  private:
    std::vector<Transcript> transcripts_;
    EquivalenceClassBuilder eqBuilder_;
    std::atomic<uint64_t> numMappedFragments_{0}, numObservedFragments_{0};
    std::string seq_; std::vector<uint64_t> seqOff_;
    std::vector<uint32_t> fld_;
    std::vector<uint32_t> readBias_ = std::vector<uint32_t>(4096, 1), observedGC_ = std::vector<uint32_t>(101, 1);
    std::vector<double> expectedSeqBias_ = std::vector<double>(4096, 1.0), expectedGC_ = std::vector<double>(101, 1.0);
    std::atomic<int64_t> numFwd_{0}, numRC_{0};
};

// ---- loadEquivClasses, src/SailfishQuantify.cpp:1444-1494 (commented out in the reference; --readEqClasses :1114) ------------
// Reads the file writeEquivCounts writes (src/GZipWriter.cpp:51-92): M, C, the M names, then C lines "k \t id_1 .. id_k \t count".
// The names must be readExp.transcripts()' names in order; the class section is parsed on the device and folded into the
// builder with upsert semantics (sfgpu_eq_add_text_host: format, limits and error kinds in sfgpu.h).  Call it between the
// builder's start() and finish(); several files fold into one table.  As the reference's loader, every count adds to the
// observed and the mapped fragments.  Throws std::runtime_error naming the file and its 1-based line.
inline void loadEquivClasses(const std::string& eqClassFile, ReadExperiment& readExp) {
    std::ifstream in(eqClassFile, std::ios::binary);
    if (!in) throw std::runtime_error(eqClassFile + ": cannot open");
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    size_t pos = 0;
    uint64_t lineno = 0;
    auto fail = [&](uint64_t line, const std::string& what) {
        throw std::runtime_error(eqClassFile + ", line " + std::to_string(line) + ": " + what);
    };
    auto next_line = [&]() -> std::string {
        ++lineno;
        const size_t e = text.find('\n', pos);
        if (e == std::string::npos) fail(lineno, "the file ends inside the header");
        std::string s = text.substr(pos, e - pos);
        pos = e + 1;
        return s;
    };
    auto number = [&](const std::string& s) -> uint64_t {
        if (s.empty() || s.size() > 19 || s.find_first_not_of("0123456789") != std::string::npos) fail(lineno, "expected a decimal integer");
        return std::stoull(s);
    };
    auto& txps = readExp.transcripts();
    const uint64_t M = number(next_line());
    if (M != txps.size()) fail(lineno, "the header lists M=" + std::to_string(M) + " transcripts, expected " + std::to_string(txps.size()));
    const uint64_t C = number(next_line());
    for (uint64_t i = 0; i < M; ++i) {
        const std::string name = next_line();
        if (name != txps[i].RefName) fail(lineno, "transcript " + std::to_string(i) + " is named '" + name + "', expected '" + txps[i].RefName + "'");
    }
    sfgpu_eqtext_result r;
    const int rc = sfgpu_eq_add_text_host(readExp.equivalenceClassBuilder().handle(), text.data() + pos, text.size() - pos, M, 0, &r);
    if (rc != SFGPU_OK) {
        if (r.err_line != UINT64_MAX) fail(2 + M + r.err_line + 1, sfgpu_last_error());
        check(rc, "sfgpu_eq_add_text_host");
    }
    if (r.n_lines != C)
        fail(2 + M + (r.n_lines < C ? r.n_lines : C) + 1, "the header announces C=" + std::to_string(C) + " classes, the file holds " +
             std::to_string(r.n_lines));
    readExp.numObservedFragmentsAtomic() += r.sum_counts;       // numObservedFragments += count; validHits += count (:1478-1479)
    readExp.numMappedFragmentsAtomic() += r.sum_counts;
}

// ---- GZipWriter::writeEquivCounts, src/GZipWriter.cpp:51-92 ----------------------------------------------------------------
// Writes the file loadEquivClasses reads: M, C and the names of readExp.transcripts() from the host, then the class lines of the
// finished builder (call it after finish()), formatted on the device from the exported table (sfgpu_eqvec_write_text: format and
// limits in sfgpu.h) and streamed into the file chunk by chunk -- no per-class vectors on the host (eqVec() is not called).
// Classes are in the canonical order.  Throws std::runtime_error naming the file when it cannot be opened or written.
inline bool writeEquivCounts(const std::string& eqClassFile, ReadExperiment& readExp) {
    std::ofstream out(eqClassFile, std::ios::binary);
    if (!out) throw std::runtime_error(eqClassFile + ": cannot open for writing");
    auto& txps = readExp.transcripts();
    auto& eq = readExp.equivalenceClassBuilder();
    const uint64_t C = eq.numClasses();
    out << txps.size() << '\n' << C << '\n';
    for (const auto& t : txps) out << t.RefName << '\n';
    if (C) {
        DeviceBuf<uint32_t> rowptr(C + 1), ids(eq.numNonzeros());
        DeviceBuf<uint64_t> counts(C);
        check(sfgpu_eq_export_device(eq.handle(), rowptr.get(), ids.get(), counts.get(), nullptr), "sfgpu_eq_export_device");
        check_hip(hipDeviceSynchronize(), "hipDeviceSynchronize");        // the export runs on the builder's stream
        auto sink = [](const char* bytes, uint64_t n, void* user) -> int {
            std::ofstream& o = *static_cast<std::ofstream*>(user);
            o.write(bytes, static_cast<std::streamsize>(n));
            return o ? 0 : 1;
        };
        sfgpu_eqtext_write_result r;
        const int rc = sfgpu_eqvec_write_text(rowptr.get(), ids.get(), counts.get(), C, 0, sink, &out, &r, nullptr);
        if (rc == SFGPU_ERR_IO) throw std::runtime_error(eqClassFile + ": write failed");
        check(rc, "sfgpu_eqvec_write_text");
    }
    out.close();
    if (!out) throw std::runtime_error(eqClassFile + ": write failed");
    return true;
}

// ---- what writeAbundances and aggregateEstimatesToGeneLevel share ------------------------------------------------------------
namespace detail {
// the columns of quant.sf on the device, as writeAbundances writes them and aggregateEstimatesToGeneLevel folds them
struct AbundanceColumns {
    uint64_t M = 0;
    DeviceBuf<char> names;
    DeviceBuf<uint64_t> off;
    DeviceBuf<uint32_t> len;
    DeviceBuf<double> eff, cnt, tpm;
    AbundanceColumns(ReadExperiment& readExp, const SailfishOpts& sopt) {
        auto& txps = readExp.transcripts();
        M = txps.size();
        if (!M) return;
        std::vector<char> h_names;
        std::vector<uint64_t> h_off(M + 1, 0);
        std::vector<uint32_t> h_len(M);
        std::vector<double> h_eff(M), h_cnt(M);
        for (uint64_t i = 0; i < M; ++i) {
            h_names.insert(h_names.end(), txps[i].RefName.begin(), txps[i].RefName.end());
            h_off[i + 1] = h_names.size();
            h_len[i] = txps[i].RefLength;
            h_eff[i] = sopt.noEffectiveLengthCorrection ? static_cast<double>(txps[i].RefLength) : txps[i].EffectiveLength;
            h_cnt[i] = txps[i].estCount();
        }
        names.resize(h_names.size()); names.upload(h_names);
        off.resize(M + 1); off.upload(h_off);
        len.resize(M); len.upload(h_len);
        eff.resize(M); eff.upload(h_eff);
        cnt.resize(M); cnt.upload(h_cnt);
        tpm.resize(M);
        check(sfgpu_tpm(cnt.get(), eff.get(), M, static_cast<double>(readExp.numMappedFragments()), tpm.get(), nullptr), "sfgpu_tpm");
    }
};
inline int ofstream_sink(const char* bytes, uint64_t n, void* user) {
    std::ofstream& o = *static_cast<std::ofstream*>(user);
    o.write(bytes, static_cast<std::streamsize>(n));
    return o ? 0 : 1;
}
}  // namespace detail

// ---- GZipWriter::writeAbundances, src/GZipWriter.cpp:194-248 ------------------------------------------------------------------
// quant.sf: the header line from the host, then one row per transcript of readExp -- Name, Length, EffectiveLength (the
// reference length with sopt.noEffectiveLengthCorrection), TPM (sfgpu_tpm over estCount()) and NumReads (estCount()) -- formatted
// on the device (sfgpu_quant_write_text: format and limits in sfgpu.h; the doubles print as the reference's "{}", printf %g) and
// streamed into the file chunk by chunk.  Throws std::runtime_error naming the file when it cannot be opened or written.
inline bool writeAbundances(const std::string& quantFile, ReadExperiment& readExp, const SailfishOpts& sopt) {
    std::ofstream out(quantFile, std::ios::binary);
    if (!out) throw std::runtime_error(quantFile + ": cannot open for writing");
    out << "Name\tLength\tEffectiveLength\tTPM\tNumReads\n";
    detail::AbundanceColumns c(readExp, sopt);
    if (c.M) {
        sfgpu_quant_write_result r;
        const int rc = sfgpu_quant_write_text(c.names.get(), c.off.get(), c.len.get(), c.eff.get(), c.tpm.get(), c.cnt.get(), c.M, 0,
                                              detail::ofstream_sink, &out, &r, nullptr);
        if (rc == SFGPU_ERR_IO) throw std::runtime_error(quantFile + ": write failed");
        check(rc, "sfgpu_quant_write_text");
    }
    out.close();
    if (!out) throw std::runtime_error(quantFile + ": write failed");
    return true;
}

// ---- aggregateEstimatesToGeneLevel, src/SailfishUtils.cpp:929-1037 (the `--geneMap` step) ------------------------------------
// quant.genes.sf at `genesFile` from the columns writeAbundances writes for readExp and sopt, without reading quant.sf back: the
// header line of quant.sf from the host, then one row per gene -- Name, Length, EffectiveLength, TPM, NumReads, in order of each
// gene's first transcript -- folded from the PRINTED values (six-digit %g tokens read back, as the reference reads them from the
// file) and formatted on the device (sfgpu_genes_aggregate / sfgpu_genes_write_text: arithmetic, order and limits in sfgpu.h).
// `geneName` maps a transcript name to its gene's name -- what TranscriptGeneMap::geneName is (lower_bound, no equality test;
// past the last name a transcript is its own gene); gene identity is the name it returns.  Throws std::runtime_error naming the
// file when it cannot be opened or written.
template <typename GeneNameOf>
inline bool aggregateEstimatesToGeneLevel(GeneNameOf&& geneName, ReadExperiment& readExp, const SailfishOpts& sopt, const std::string& genesFile) {
    std::ofstream out(genesFile, std::ios::binary);
    if (!out) throw std::runtime_error(genesFile + ": cannot open for writing");
    out << "Name\tLength\tEffectiveLength\tTPM\tNumReads\n";
    detail::AbundanceColumns c(readExp, sopt);
    if (c.M) {
        auto& txps = readExp.transcripts();
        std::unordered_map<std::string, uint32_t> idOf;
        std::vector<char> gNames;
        std::vector<uint64_t> gOff(1, 0);
        std::vector<uint32_t> geneOfRow(c.M);
        for (uint64_t i = 0; i < c.M; ++i) {
            const std::string g = geneName(txps[i].RefName);
            auto it = idOf.find(g);
            if (it == idOf.end()) {
                it = idOf.emplace(g, static_cast<uint32_t>(idOf.size())).first;
                gNames.insert(gNames.end(), g.begin(), g.end());
                gOff.push_back(gNames.size());
            }
            geneOfRow[i] = it->second;
        }
        const uint64_t G = idOf.size();
        DeviceBuf<uint32_t> dGeneOfRow(geneOfRow), dGeneId(G);
        DeviceBuf<char> dNames(gNames);
        DeviceBuf<uint64_t> dOff(gOff);
        DeviceBuf<double> gLen(G), gEff(G), gTpm(G), gCnt(G);
        sfgpu_genes_result ar;
        check(sfgpu_genes_aggregate(dGeneOfRow.get(), c.len.get(), c.eff.get(), c.tpm.get(), c.cnt.get(), c.M, G, 1, dGeneId.get(), gLen.get(),
                                    gEff.get(), gTpm.get(), gCnt.get(), &ar, nullptr), "sfgpu_genes_aggregate");
        sfgpu_quant_write_result r;
        const int rc = sfgpu_genes_write_text(dNames.get(), dOff.get(), G, dGeneId.get(), gLen.get(), gEff.get(), gTpm.get(), gCnt.get(),
                                              ar.n_genes, 0, detail::ofstream_sink, &out, &r, nullptr);
        if (rc == SFGPU_ERR_IO) throw std::runtime_error(genesFile + ": write failed");
        check(rc, "sfgpu_genes_write_text");
    }
    out.close();
    if (!out) throw std::runtime_error(genesFile + ": write failed");
    return true;
}

// ---- TranscriptGeneMap read and joined on the device (sfgpu_gmap_*) ----------------------------------------------------------
// The map of a --geneMap file as a device handle: sorted transcript names, t2g and gene names (include/TranscriptGeneMap.hpp),
// built by readTranscriptToGeneMap below.
class DeviceGeneMap {
  public:
    DeviceGeneMap(int kind, const std::string& key) { check(sfgpu_gmap_open(&h_, kind, key.data(), static_cast<uint32_t>(key.size())), "sfgpu_gmap_open"); }
    DeviceGeneMap(const DeviceGeneMap&) = delete;
    DeviceGeneMap& operator=(const DeviceGeneMap&) = delete;
    ~DeviceGeneMap() { (void)sfgpu_gmap_close(h_); }
    sfgpu_gmap* get() const { return h_; }
    uint64_t numTranscripts() const { return info.n_transcripts; }
    uint64_t numGenes() const { return info.n_genes; }
    sfgpu_gmap_result info = sfgpu_gmap_result();      // filled by finish
  private:
    sfgpu_gmap* h_ = nullptr;
};

// readTranscriptToGeneMap / transcriptGeneMapFromGTF (src/SailfishUtils.cpp:322-507): a file whose extension is .gtf is read as GTF
// (`key` names the attribute that groups transcripts), anything else as `transcript gene` pairs.  The file goes to the device
// block by block (sfgpu_gmap_add_text_host; the unconsumed tail of a block is carried in front of the next) and is parsed,
// sorted and numbered there.  Throws std::runtime_error when the file cannot be read, or holds what the device rules do not
// parse (a non-ASCII byte, a NUL, a lone '\r', a name longer than 256 bytes: sfgpu.h) -- this adaptor has no host reader.
// A gzip-compressed map is not inflated here (the Python side does that): its bytes are flagged and refused like any other
// non-text.  blockBytes is cut to the 2^30 bytes one call takes.
inline std::unique_ptr<DeviceGeneMap> readTranscriptToGeneMap(const std::string& path, const std::string& key = "gene_id",
                                                              size_t blockBytes = size_t(32) << 20) {
    std::ifstream in(path, std::ios::binary);
    if (!in) throw std::runtime_error(path + ": cannot open the gene map");
    const bool gtf = path.size() >= 4 && path.compare(path.size() - 4, 4, ".gtf") == 0;
    std::unique_ptr<DeviceGeneMap> m(new DeviceGeneMap(gtf ? SFGPU_GMAP_GTF : SFGPU_GMAP_TSV, key));
    if (blockBytes > (size_t(1) << 29)) blockBytes = size_t(1) << 29;      // a block and the tail in front of it: one call takes 2^30 bytes
    std::vector<char> buf;
    bool eof = false;
    while (!eof) {
        const size_t had = buf.size();
        buf.resize(had + (blockBytes ? blockBytes : 1));
        in.read(buf.data() + had, static_cast<std::streamsize>(buf.size() - had));
        buf.resize(had + static_cast<size_t>(in.gcount()));
        eof = in.eof();
        if (in.bad()) throw std::runtime_error(path + ": read failed");
        sfgpu_gmap_add_result r;
        const int rc = sfgpu_gmap_add_text_host(m->get(), buf.data(), buf.size(), eof ? 1 : 0, &r, nullptr);
        if (rc == SFGPU_ERR_RANGE && r.consumed == 0 && !eof && buf.size() < (size_t(1) << 30)) continue;      // no line ends yet: read on
        check(rc, "sfgpu_gmap_add_text_host");
        if (r.needs_host) throw std::runtime_error(path + ": the gene map holds bytes the device reader does not parse");
        buf.erase(buf.begin(), buf.begin() + static_cast<std::ptrdiff_t>(r.consumed));
    }
    check(sfgpu_gmap_finish(m->get(), &m->info, nullptr), "sfgpu_gmap_finish");
    return m;
}

// aggregateEstimatesToGeneLevel with the map on the device: the transcript names of readExp are joined to it there
// (sfgpu_gmap_lookup: TranscriptGeneMap::findTranscriptID, lower_bound with no equality test) and the gene names are written from
// the map's own table.  Only when a transcript sorts past the map's last name -- it is then its own gene, keyed by its name --
// are the ids of those rows resolved on the host.  The file is the one the functor form writes with tgm.geneName.
inline bool aggregateEstimatesToGeneLevel(const DeviceGeneMap& tgm, ReadExperiment& readExp, const SailfishOpts& sopt, const std::string& genesFile) {
    std::ofstream out(genesFile, std::ios::binary);
    if (!out) throw std::runtime_error(genesFile + ": cannot open for writing");
    out << "Name\tLength\tEffectiveLength\tTPM\tNumReads\n";
    detail::AbundanceColumns c(readExp, sopt);
    if (c.M) {
        uint64_t G = tgm.numGenes(), nPast = 0;
        DeviceBuf<uint32_t> dGeneOfRow(c.M);
        check(sfgpu_gmap_lookup(tgm.get(), c.names.get(), c.off.get(), c.M, dGeneOfRow.get(), &nPast, nullptr), "sfgpu_gmap_lookup");
        DeviceBuf<char> dNames(static_cast<size_t>(tgm.info.gname_bytes));
        DeviceBuf<uint64_t> dOff(static_cast<size_t>(G + 1));
        check(sfgpu_gmap_export(tgm.get(), nullptr, nullptr, nullptr, dNames.get(), dOff.get(), nullptr), "sfgpu_gmap_export");
        if (nPast) {
            std::vector<char> gNames = dNames.download();
            std::vector<uint64_t> gOff = dOff.download();
            std::vector<uint32_t> geneOfRow = dGeneOfRow.download();
            std::unordered_map<std::string, uint32_t> idOf;
            for (uint64_t g = 0; g < G; ++g) idOf.emplace(std::string(gNames.data() + gOff[g], gNames.data() + gOff[g + 1]), static_cast<uint32_t>(g));
            auto& txps = readExp.transcripts();
            for (uint64_t i = 0; i < c.M; ++i) {
                if (geneOfRow[i] != 0xFFFFFFFFu) continue;
                const std::string& g = txps[i].RefName;
                auto it = idOf.find(g);
                if (it == idOf.end()) {
                    it = idOf.emplace(g, static_cast<uint32_t>(gOff.size() - 1)).first;
                    gNames.insert(gNames.end(), g.begin(), g.end());
                    gOff.push_back(gNames.size());
                }
                geneOfRow[i] = it->second;
            }
            G = gOff.size() - 1;
            dGeneOfRow.upload(geneOfRow);
            dNames.resize(gNames.size()); dNames.upload(gNames);
            dOff.resize(gOff.size()); dOff.upload(gOff);
        }
        const size_t cap = static_cast<size_t>(G < c.M ? G : c.M);
        DeviceBuf<uint32_t> dGeneId(cap);
        DeviceBuf<double> gLen(cap), gEff(cap), gTpm(cap), gCnt(cap);
        sfgpu_genes_result ar;
        check(sfgpu_genes_aggregate(dGeneOfRow.get(), c.len.get(), c.eff.get(), c.tpm.get(), c.cnt.get(), c.M, G, 1, dGeneId.get(), gLen.get(),
                                    gEff.get(), gTpm.get(), gCnt.get(), &ar, nullptr), "sfgpu_genes_aggregate");
        sfgpu_quant_write_result r;
        const int rc = sfgpu_genes_write_text(dNames.get(), dOff.get(), G, dGeneId.get(), gLen.get(), gEff.get(), gTpm.get(), gCnt.get(),
                                              ar.n_genes, 0, detail::ofstream_sink, &out, &r, nullptr);
        if (rc == SFGPU_ERR_IO) throw std::runtime_error(genesFile + ": write failed");
        check(rc, "sfgpu_genes_write_text");
    }
    out.close();
    if (!out) throw std::runtime_error(genesFile + ": write failed");
    return true;
}
inline bool aggregateEstimatesToGeneLevel(DeviceGeneMap& tgm, ReadExperiment& readExp, const SailfishOpts& sopt, const std::string& genesFile) {
    return aggregateEstimatesToGeneLevel(static_cast<const DeviceGeneMap&>(tgm), readExp, sopt, genesFile);
}

// ---- GZipWriter::writeBootstrap<T>, src/GZipWriter.cpp:249-285 ----------------------------------------------------------------
// The reference appends every sample to one boost gzip stream on the host.  Here the samples stay where sfgpu_bootstrap /
// sfgpu_gibbs_sample left them (d_out: n_samples x M elements of elem_bytes, rows in draw order) and are compressed on the device
// (sfgpu_gz_*: one gzip member, payload = the raw little-endian samples); the file is what gzip readers expect of bootstraps.gz.
// Throws std::runtime_error naming the file when it cannot be opened or written.
inline bool writeBootstraps(const std::string& bsFile, const void* d_samples, uint64_t n_samples, uint64_t M, uint64_t elem_bytes) {
    std::ofstream out(bsFile, std::ios::binary);
    if (!out) throw std::runtime_error(bsFile + ": cannot open for writing");
    auto sink = [](const char* bytes, uint64_t n, void* user) -> int {
        std::ofstream& o = *static_cast<std::ofstream*>(user);
        o.write(bytes, static_cast<std::streamsize>(n));
        return o ? 0 : 1;
    };
    sfgpu_gz* z = nullptr;
    int rc = sfgpu_gz_open(&z, sink, &out, 0);
    if (rc == SFGPU_OK) {
        const int rc_w = sfgpu_gz_write_device(z, d_samples, n_samples * M * elem_bytes, nullptr);
        rc = sfgpu_gz_close(z, nullptr);              // frees the handle whatever happened
        if (rc_w != SFGPU_OK) rc = rc_w;
    }
    if (rc == SFGPU_ERR_IO) throw std::runtime_error(bsFile + ": write failed");
    check(rc, "sfgpu_gz_write_device");
    out.close();
    if (!out) throw std::runtime_error(bsFile + ": write failed");
    return true;
}

namespace detail {
inline Logger* active_logger(Logger* set = nullptr, bool clear = false) {
    static Logger* cur = nullptr;
    if (set) cur = set;
    if (clear) cur = nullptr;
    return cur;
}
inline void log_trampoline(int level, const char* msg) { if (Logger* l = active_logger()) if (*l) (*l)(level, msg); }
struct LoggerScope {       // the library logs what the reference logs (iteration lines, class counts) through jointLog
    explicit LoggerScope(Logger& l) { if (l) { active_logger(&l); sfgpu_set_logger(log_trampoline); } }
    ~LoggerScope() { active_logger(nullptr, true); sfgpu_set_logger(nullptr); }
};

// the device-side problem of one experiment: lengths + the builder's classes (never leave HBM)
struct DeviceProblem {
    DeviceBuf<double> len;
    DeviceBuf<uint32_t> rowptr, ids;
    DeviceBuf<uint64_t> counts;
    sfgpu_problem prob{};
    DeviceProblem(ReadExperiment& readExp, const SailfishOpts& sopt) {
        auto& txps = readExp.transcripts();
        auto& eq = readExp.equivalenceClassBuilder();
        std::vector<double> h(txps.size());
        for (size_t i = 0; i < txps.size(); ++i)                                   // src/CollapsedEMOptimizer.cpp:736-737
            h[i] = sopt.noEffectiveLengthCorrection ? static_cast<double>(txps[i].RefLength) : txps[i].EffectiveLength;
        len.resize(h.size()); len.upload(h);
        rowptr.resize(eq.numClasses() + 1); ids.resize(eq.numNonzeros()); counts.resize(eq.numClasses());
        check(sfgpu_eq_export_device(eq.handle(), rowptr.get(), ids.get(), counts.get(), nullptr), "sfgpu_eq_export_device");
        prob = sfgpu_problem{txps.size(), len.get(), eq.numClasses(), rowptr.get(), ids.get(), counts.get(), readExp.numMappedFragments()};
    }
};
}  // namespace detail

// ---- include/CollapsedEMOptimizer.hpp:20-35 ----------------------------------------------------------------
class CollapsedEMOptimizer {
  public:
    CollapsedEMOptimizer() = default;

    // src/CollapsedEMOptimizer.cpp:711-893.  false where the reference logs an error and returns false
    // ("no transcripts expressed" :794-798, "total alpha weight was too small" :877-881).
    bool optimize(ReadExperiment& readExp, SailfishOpts& sopt, double tolerance = 0.01, uint32_t maxIter = 1000) {
        const bool doBiasCorrect = sopt.biasCorrect || sopt.gcBiasCorrect;         // :717
        detail::LoggerScope scope(sopt.jointLog);
        auto& txps = readExp.transcripts();
        const uint64_t M = txps.size();
        detail::DeviceProblem dp(readExp, sopt);
        DeviceBuf<double> alpha(M), mass(M);
        sfgpu_em* em = nullptr;
        check(sfgpu_em_create(&em, &dp.prob, nullptr), "sfgpu_em_create");
        sfgpu_em_opts o{sopt.useVBOpt ? 1 : 0, tolerance, /*minIter :716*/ 50, maxIter, /*check_mode*/ 0, 0};
        sfgpu_em_stats st{};
        int rc;
        std::vector<double> newEffLens;
        lastRecomputes = 0;
        if (doBiasCorrect) {
            // everything updateEffectiveLengths reads from the experiment (src/SailfishUtils.cpp:611-690), then the
            // loop with the recompute hook (:814-840); the corrected lengths come back for :888
            std::vector<char> seq(readExp.sequences().begin(), readExp.sequences().end());
            std::vector<uint32_t> refLens(M); std::vector<double> txpEff(M);
            for (uint64_t i = 0; i < M; ++i) { refLens[i] = txps[i].RefLength; txpEff[i] = txps[i].EffectiveLength; }
            DeviceBuf<char> dSeq(seq); DeviceBuf<uint64_t> dOff(readExp.sequenceOffsets());
            DeviceBuf<uint32_t> dRef(refLens); DeviceBuf<double> dTxpEff(txpEff), dEffOut(M);
            sfgpu_bias_inputs bi{};
            bi.M = M; bi.d_seq = dSeq.get(); bi.d_seq_off = dOff.get(); bi.d_ref_len = dRef.get(); bi.d_txp_eff_len = dTxpEff.get();
            bi.h_fl_counts = readExp.fragLengthCounts().data(); bi.max_frag_len = static_cast<uint32_t>(readExp.fragLengthCounts().size());
            bi.gc_speed_samp = sopt.pdfSampFactor; bi.h_read_bias = readExp.readBias().data(); bi.h_observed_gc = readExp.observedGC().data();
            bi.num_fwd = readExp.numFwd(); bi.num_rc = readExp.numRC();
            bi.seq_bias = sopt.biasCorrect; bi.gc_bias = sopt.gcBiasCorrect; bi.gc_size_samp = sopt.gcSampFactor;
            sfgpu_bias* bias = nullptr;
            rc = sfgpu_bias_create(&bias, &bi, nullptr);
            if (rc != SFGPU_OK) { sfgpu_em_destroy(em); check(rc, "sfgpu_bias_create"); }
            rc = sfgpu_em_optimize_bias(em, &o, bias, alpha.get(), mass.get(), dEffOut.get(), &lastRecomputes, &st);
            if (rc == SFGPU_OK) {
                (void)sfgpu_bias_expected(bias, readExp.expectedSeqBias().data(), readExp.expectedGCBias().data());
                newEffLens = dEffOut.download();
            }
            sfgpu_bias_destroy(bias);
        } else {
            rc = sfgpu_em_optimize(em, &o, alpha.get(), mass.get(), &st);
        }
        sfgpu_em_destroy(em);
        lastIterations = st.iters;
        if (rc == SFGPU_ERR_NO_ACTIVE || rc == SFGPU_ERR_ALPHA_SUM) return false;
        check(rc, "sfgpu_em_optimize");
        for (size_t i = 0; i < newEffLens.size(); ++i) txps[i].EffectiveLength = newEffLens[i];   // :888
        const std::vector<double> a = alpha.download(), m = mass.download();
        std::vector<uint32_t> members = dp.ids.download();
        for (uint32_t t : members) txps[t].setActive();                            // :774-782
        for (size_t i = 0; i < txps.size(); ++i) { txps[i].setEstCount(a[i]); txps[i].setMass(m[i]); }   // :885-891
        return true;
    }

    // src/CollapsedEMOptimizer.cpp:557-709 (doBootstrap :438-525).  The reference seeds from std::random_device.
    bool gatherBootstraps(ReadExperiment& readExp, SailfishOpts& sopt,
                          std::function<bool(const std::vector<double>&)>& writeBootstrap,
                          double relDiffTolerance, uint32_t maxIter) {
        detail::LoggerScope scope(sopt.jointLog);
        detail::DeviceProblem dp(readExp, sopt);
        sfgpu_em* em = nullptr;
        check(sfgpu_em_create(&em, &dp.prob, nullptr), "sfgpu_em_create");
        sfgpu_em_opts o{sopt.useVBOpt ? 1 : 0, relDiffTolerance, /*min_iter*/ 0, maxIter, /*check_mode :499*/ 1, 0};
        struct Ctx { std::function<bool(const std::vector<double>&)>* w; } ctx{&writeBootstrap};
        auto cb = [](const double* a, uint64_t M, void* user) -> int {
            std::vector<double> v(a, a + M);
            return (*static_cast<Ctx*>(user)->w)(v) ? 1 : 0;
        };
        std::random_device rd;
        const uint64_t seed = (static_cast<uint64_t>(rd()) << 32) | rd();
        const int rc = sfgpu_bootstrap(em, &o, sopt.numBootstraps, seed, nullptr, cb, &ctx, nullptr);
        sfgpu_em_destroy(em);
        if (rc == SFGPU_ERR_NO_ACTIVE || rc == SFGPU_ERR_ALPHA_SUM) return false;
        check(rc, "sfgpu_bootstrap");
        return true;
    }

    uint32_t lastIterations = 0;       // the N of the reference's log line "iteration = N | max rel diff. = x" (:871-872)
    uint32_t lastRecomputes = 0;       // how often "recomputing effective lengths" (:827) happened
};

// ---- include/CollapsedGibbsSampler.hpp:22-32 ---------------------------------------------------------------
class CollapsedGibbsSampler {
  public:
    CollapsedGibbsSampler() = default;
    // src/CollapsedGibbsSampler.cpp:187-291; reads Transcript::mass() as optimize() left it (it does not overwrite
    // it, unlike :219-221)
    bool sample(ReadExperiment& readExp, SailfishOpts& sopt, std::function<bool(const std::vector<int>&)>& writeBootstrap,
                uint32_t numSamples = 500) {
        detail::LoggerScope scope(sopt.jointLog);
        auto& txps = readExp.transcripts();
        detail::DeviceProblem dp(readExp, sopt);
        std::vector<double> m(txps.size());
        for (size_t i = 0; i < txps.size(); ++i) m[i] = txps[i].mass();
        DeviceBuf<double> mass(m);
        struct Ctx { std::function<bool(const std::vector<int>&)>* w; } ctx{&writeBootstrap};
        auto cb = [](const int32_t* c, uint64_t M, void* user) -> int {
            std::vector<int> v(c, c + M);
            return (*static_cast<Ctx*>(user)->w)(v) ? 1 : 0;
        };
        std::random_device rd;
        const uint64_t seed = (static_cast<uint64_t>(rd()) << 32) | rd();
        const int rc = sfgpu_gibbs_sample(&dp.prob, mass.get(), numSamples, 0, seed, nullptr, cb, &ctx, nullptr);
        if (rc != SFGPU_OK) { if (sopt.jointLog) sopt.jointLog(2, sfgpu_last_error()); return false; }
        return true;
    }
};

}  // namespace gpu
}  // namespace sailfish
#endif  // SFGPU_SAILFISH_HPP
