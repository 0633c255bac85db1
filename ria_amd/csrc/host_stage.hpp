// ria_amd/csrc/host_stage.hpp — the staging block of a host-buffer call, laid out with the Carver.  Plain C++17, no HIP:
// tests/helpers/host_stage_check.cpp builds it with g++.
//
// A host-buffer call fills the inputs of a pinned block, sends them to a device block of the same layout in one copy, runs
// the batch form there, brings the outputs back in one copy and hands them to the caller.  The layout is written once, as
// a function that walks a StageCarver with the caller's own pointers and returns a struct of typed pointers into the
// block, every input before the first output:
//     FooStage w; w.x = c.in(n, x_host); w.meta = c.in(n, meta_host); w.llr = c.out(n, llr_out_host); w.st = c.out(n, st_out_host);
// On a null base the walk gives the size of the block and the two copies, on the device block the batch form's pointers,
// on the pinned block fill() and drain():
//     host -> device   bytes [0, upload_end()):           to the end of the last input that is present; never an output
//     device -> host   bytes [download_begin(), size()):  from the first output that is wanted to the end of the block
// An optional area (a null host pointer) keeps its place.  An input declared behind an output would sit in the wrong
// copy, and more than kMaxAreas of a kind are not recorded: the walk is then not valid(), and the caller refuses to run.
#pragma once
#include <cstring>

#include "ws_carve.hpp"

namespace ria {

class StageCarver {
public:
    static constexpr int kMaxAreas = 8;
    explicit StageCarver(void* base = nullptr) : c_(base) {}
    // `count` elements: the first n_copy (default: all) come from src, the rest are zero.  src null: the input is absent -
    // not filled, uploaded only if a present input follows - and so is the pointer (the batch form's "not given").
    template <typename T>
    T* in(size_t count, const T* src, size_t n_copy = kAll) {
        if (first_out_ != kAll || n_in_ == kMaxAreas) { valid_ = false; return nullptr; }
        const size_t at = c_.offset();
        T* p = c_.take<T>(count);
        if (!src) return nullptr;
        upload_end_ = at + count * sizeof(T);
        in_[n_in_++] = {p, src, (n_copy < count ? n_copy : count) * sizeof(T), count * sizeof(T)};
        return p;
    }
    // `count` elements, of which drain() hands the first n_copy (default: all) to dst.  dst null: nobody reads the output;
    // the batch form writes it all the same, and the download starts at the first output that somebody reads.
    template <typename T>
    T* out(size_t count, T* dst, size_t n_copy = kAll) {
        if (n_out_ == kMaxAreas) { valid_ = false; return nullptr; }
        if (first_out_ == kAll) first_out_ = c_.offset();
        if (dst && download_begin_ == kAll) download_begin_ = c_.offset();
        T* p = c_.take<T>(count);
        if (dst) out_[n_out_++] = {p, dst, (n_copy < count ? n_copy : count) * sizeof(T)};
        return p;
    }
    void fill() const {    // on the pinned block, before the upload
        for (int i = 0; i < n_in_; ++i) {
            std::memcpy(in_[i].area, in_[i].src, in_[i].bytes);
            std::memset(static_cast<char*>(in_[i].area) + in_[i].bytes, 0, in_[i].area_bytes - in_[i].bytes);
        }
    }
    void drain() const {   // on the pinned block, after the download
        for (int i = 0; i < n_out_; ++i) std::memcpy(out_[i].dst, out_[i].area, out_[i].bytes);
    }
    bool valid() const { return valid_; }
    size_t size() const { return c_.offset(); }
    size_t upload_end() const { return upload_end_; }
    size_t first_output() const { return first_out_ == kAll ? size() : first_out_; }
    size_t download_begin() const { return download_begin_ == kAll ? size() : download_begin_; }
private:
    static constexpr size_t kAll = ~size_t(0);
    struct In { void* area; const void* src; size_t bytes, area_bytes; };
    struct Out { const void* area; void* dst; size_t bytes; };
    Carver c_;
    In in_[kMaxAreas];
    Out out_[kMaxAreas];
    int n_in_ = 0, n_out_ = 0;
    size_t upload_end_ = 0, first_out_ = kAll, download_begin_ = kAll;
    bool valid_ = true;
};

}  // namespace ria
