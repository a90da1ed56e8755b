// csrc/pair_book.h — the pair book: what is method-independent about a batch of alignments.  Which clouds are the targets, which (target, source, guess)
// pairs are to be aligned, and the device copies of the clouds that came as host pointers.  A plain host class: no engine state, no kernels.  The engines
// (NdtEngine, GicpBatch) and the fitness passes read it; mrgfe_batch and mrgfe_reg own one next to their engines.
#pragma once
#include <cstring>
#include <vector>

#include "common.h"

namespace mrgfe {

class PairBook {
   public:
    struct Target { const float4* d_pts = nullptr; uint32_t n = 0; };
    struct Pair { int target = -1; const float4* d_src = nullptr; uint32_t n = 0; float guess[16]; /* row-major */ };

    explicit PairBook(mrgfe_ctx* ctx) : ctx_(ctx) {}
    ~PairBook() { if (ctx_) (void)hipSetDevice(ctx_->device); }  // the arena frees itself on the book's device

    void clear() { targets_.clear(); pairs_.clear(); cloud_arena_.reset(); ++revision_; }  // forget targets and pairs (device memory is kept for reuse)
    void clear_pairs() { pairs_.clear(); ++revision_; }
    // clouds: host (strided) or device (packed float4). device clouds are referenced, not copied.
    int add_target_device(const void* d_xyzi, size_t n)
    {
        if (n > 0 && !d_xyzi) { set_error("add_target: NULL cloud"); return MRGFE_ERR_INVALID; }
        if (n > 0x7fffffffu) { set_error("add_target: cloud too large"); return MRGFE_ERR_INVALID; }
        targets_.push_back(Target{static_cast<const float4*>(d_xyzi), static_cast<uint32_t>(n)});
        ++revision_;
        return n_targets() - 1;
    }
    int add_target_host(const float* xyzi, size_t n, size_t stride)
    {
        if (n > 0 && !xyzi) { set_error("add_target: NULL cloud"); return MRGFE_ERR_INVALID; }
        void* d = nullptr;
        MRGFE_TRY(upload(xyzi, n, stride, &d));
        return add_target_device(d, n);
    }
    int add_pair_device(int target, const void* d_xyzi, size_t n, const float guess_rowmajor[16])
    {
        if (target < 0 || target >= n_targets()) { set_error("add_pair: target index %d out of range", target); return MRGFE_ERR_INVALID; }
        if (n > 0 && !d_xyzi) { set_error("add_pair: NULL cloud"); return MRGFE_ERR_INVALID; }
        if (n > 0x7fffffffu) { set_error("add_pair: cloud too large"); return MRGFE_ERR_INVALID; }
        Pair p;
        p.target = target;
        p.d_src = static_cast<const float4*>(d_xyzi);
        p.n = static_cast<uint32_t>(n);
        std::memcpy(p.guess, guess_rowmajor, sizeof(p.guess));
        pairs_.push_back(p);
        ++revision_;
        return n_pairs() - 1;
    }
    int add_pair_host(int target, const float* xyzi, size_t n, size_t stride, const float guess_rowmajor[16])
    {
        if (n > 0 && !xyzi) { set_error("add_pair: NULL cloud"); return MRGFE_ERR_INVALID; }
        void* d = nullptr;
        MRGFE_TRY(upload(xyzi, n, stride, &d));
        return add_pair_device(target, d, n, guess_rowmajor);
    }
    int set_guess(int pair, const float guess_rowmajor[16])
    {
        if (pair < 0 || pair >= n_pairs()) { set_error("set_guess: pair index %d out of range", pair); return MRGFE_ERR_INVALID; }
        std::memcpy(pairs_[pair].guess, guess_rowmajor, sizeof(float) * 16);
        ++revision_;
        return MRGFE_OK;
    }

    int n_targets() const { return static_cast<int>(targets_.size()); }
    int n_pairs() const { return static_cast<int>(pairs_.size()); }
    const Target& target(int i) const { return targets_[i]; }
    const Pair&   pair(int i) const { return pairs_[i]; }
    // counts every mutation above: a reader that keeps something derived from the lists (NdtEngine's device pair table) compares it with the value it saw last
    uint64_t revision() const { return revision_; }

   private:
    int upload(const float* xyzi, size_t n, size_t stride, void** d)  // a host cloud into the arena, on the context's stream
    {
        MRGFE_TRY(ctx_->bind());
        MRGFE_TRY(cloud_arena_.alloc(n * 16, d));
        return upload_cloud(ctx_, xyzi, n, stride, *d);
    }
    mrgfe_ctx* ctx_;
    std::vector<Target> targets_;
    std::vector<Pair>   pairs_;
    Arena    cloud_arena_;  // host-supplied clouds copied to the device
    uint64_t revision_ = 1;
};

}  // namespace mrgfe
