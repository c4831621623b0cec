// rsqp_batch_staging.h -- the staging block of a host-pointer call on a batch, in plain C++17 (no HIP header: tests/host/ checks it
// on the host alone). A call declares its arrays once, in order; from the declarations follow the offsets, the block's size, the
// part that comes down, the copies into and out of the block and the device addresses. rsqp_batch.h adds the HIP side (Staging).
// Below the class: the field tables of the eight calls that stage.
#pragma once
#include <cstddef>
#include <cstring>
#include <type_traits>

#include "../../include/rsqp_hip.h"

namespace rsqp_batch_units {
// The block in declaration order: doubles on 8-byte boundaries, a run of int arrays packed two to a double word (the run is
// rounded up to a whole word). UP: the caller's bytes go to the device. BOTH: they go up, so that a member that sits out keeps
// them, and come down. DOWN: they come down only. What comes down is one tail of the block, which starts on a double word: an UP
// field behind it is refused. A null array (an optional output; a required array of count 0) keeps its room, copies nothing and
// has a null device address. Nothing is allocated: the table is CAP fields on the stack, and one field more is refused.
class StagingLayout {
public:
    enum Dir { UP, BOTH, DOWN };
    static constexpr int CAP = 24;
    struct Field { void *ref, *host; size_t off, bytes; bool is_int; Dir dir; };   // ref: the pointer field; off: in bytes

    // each of `fields` holds the caller's array of `count` elements (int, or a type of whole doubles) and gets its device address
    template <class... T>
    void add(Dir dir, size_t count, T *&... fields) { (add_one(dir, count, fields), ...); }
    bool ok() const { return ok_; }                                 // every field was taken
    int count() const { return n_; }
    const Field &field(int k) const { return f_[k]; }
    size_t words() const { return round_up(bytes_) / sizeof(double); }         // doubles of the block
    size_t up_words() const { return round_up(up_bytes_) / sizeof(double); }   // the leading part that goes up
    size_t tail() const { return has_tail_ ? tail_ : words(); }                // the first double word that comes down

    // the caller's arrays into a block of words() doubles
    void pack(double *block) const {
        for (int k = 0; k < n_; k++)
            if (f_[k].dir != DOWN && f_[k].host && f_[k].bytes) std::memcpy(at(block, k), f_[k].host, f_[k].bytes);
    }
    // every declared pointer field to its place in the device's block, null where the caller's array is null
    void address(double *device) const {
        for (int k = 0; k < n_; k++) {
            void *const p = f_[k].host ? at(device, k) : nullptr;
            std::memcpy(f_[k].ref, &p, sizeof(p));
        }
    }
    // the tail of the block into the caller's arrays
    void unpack(const double *block) const {
        for (int k = 0; k < n_; k++)
            if (f_[k].dir != UP && f_[k].host && f_[k].bytes) std::memcpy(f_[k].host, at(block, k), f_[k].bytes);
    }

private:
    template <class T>
    void add_one(Dir dir, size_t count, T *&field) {
        constexpr bool is_int = std::is_same<typename std::remove_const<T>::type, int>::value;
        static_assert(is_int || sizeof(T) % sizeof(double) == 0, "a staged array holds ints or whole doubles");
        if (n_ == CAP || (dir == UP && has_tail_)) { ok_ = false; return; }
        if (!is_int || (dir != UP && !has_tail_)) bytes_ = round_up(bytes_);
        if (dir != UP && !has_tail_) { tail_ = bytes_ / sizeof(double); has_tail_ = true; }
        f_[n_++] = Field{&field, const_cast<void *>(static_cast<const void *>(field)), bytes_, count * sizeof(T), is_int, dir};
        bytes_ += count * sizeof(T);
        if (dir != DOWN) up_bytes_ = bytes_;
    }
    static size_t round_up(size_t bytes) { return (bytes + sizeof(double) - 1) / sizeof(double) * sizeof(double); }
    void *at(const double *block, int k) const { return const_cast<char *>(reinterpret_cast<const char *>(block)) + f_[k].off; }
    Field f_[CAP];
    int n_ = 0;
    size_t bytes_ = 0, up_bytes_ = 0, tail_ = 0;
    bool has_tail_ = false, ok_ = true;
};

// The field tables: nq members, sN NLP variables and sC constraints in the batch
struct StageSizes { size_t nq, sN, sC; };

// rsqp_batch_handler_update
inline void stage_iterate(StagingLayout &L, rsqp_handler_iterate &it, StageSizes z) {
    L.add(L.UP, z.nq, it.delta, it.rho);
    L.add(L.UP, z.sN, it.x_k, it.grad);
    L.add(L.UP, z.sC, it.c_k);
    L.add(L.UP, z.nq, it.what);
}
// rsqp_batch_handler_get_step
inline void stage_step(StagingLayout &L, double *&p, double *&lam_c, double *&lam_x, double *&infea_model, double *&norm_p, StageSizes z) {
    L.add(L.DOWN, z.sN, p, lam_x);
    L.add(L.DOWN, z.sC, lam_c);
    L.add(L.DOWN, z.nq, infea_model, norm_p);
}
// rsqp_batch_handler_set_matrices: nJ / nH are 0 where the array is not given, which then takes no room
inline void stage_matrices(StagingLayout &L, const int *&what, const double *&jac, const double *&hess, size_t nq, size_t nJ, size_t nH) {
    L.add(L.UP, nq, what);
    L.add(L.UP, nJ, jac);
    L.add(L.UP, nH, hess);
}
// rsqp_batch_handler_infeasibility
inline void stage_infeasibility(StagingLayout &L, const double *&c, double *&infea, StageSizes z) {
    L.add(L.UP, z.sC, c);
    L.add(L.DOWN, z.nq, infea);
}
// rsqp_batch_handler_ratio_test (rsqp_nlp_trial) and rsqp_batch_handler_soc_begin / _soc_end (rsqp_soc_trial: the former's fields
// and more). The outputs go up as well: a member that sits out keeps their bytes
template <class Trial>
inline void stage_trial(StagingLayout &L, Trial &t, StageSizes z) {
    constexpr bool soc = std::is_same<Trial, rsqp_soc_trial>::value;
    L.add(L.UP, z.nq, t.what, t.rho, t.f_trial);
    L.add(L.UP, z.sC, t.c_trial);
    if constexpr (soc) { L.add(L.UP, z.sN, t.grad); L.add(L.UP, z.nq, t.infea_model); }
    L.add(L.BOTH, z.sN, t.x_k);
    L.add(L.BOTH, z.sC, t.c_k);
    L.add(L.BOTH, z.nq, t.f_k, t.infea_k, t.delta, t.actual_reduction, t.pred_reduction, t.infea_trial);
    if constexpr (soc) { L.add(L.BOTH, z.sN, t.x_trial); L.add(L.BOTH, z.nq, t.qp_obj); }
    L.add(L.BOTH, z.nq, t.accept, t.hu_word, t.hm_word, t.exitflag);
    if constexpr (soc) L.add(L.BOTH, z.nq, t.soc, t.nwsr_soc);
}
// rsqp_batch_handler_check_optimality (a status record is whole doubles)
inline void stage_point(StagingLayout &L, rsqp_nlp_point &pt, rsqp_optimality_status *&out, int *&verdict, StageSizes z) {
    L.add(L.UP, z.nq, pt.what);
    L.add(L.UP, z.sN, pt.x_k, pt.grad);
    L.add(L.UP, z.sC, pt.c_k);
    L.add(L.UP, z.nq, pt.infea);
    L.add(L.BOTH, z.nq, out);
    L.add(L.BOTH, z.nq, verdict);
}
// rsqp_batch_handler_update_penalty
inline void stage_penalty(StagingLayout &L, rsqp_penalty_state &s, StageSizes z) {
    L.add(L.UP, z.nq, s.what, s.infea_k, s.delta);
    L.add(L.UP, z.sN, s.x_k);
    L.add(L.UP, z.sC, s.c_k);
    L.add(L.BOTH, z.nq, s.rho, s.eps1, s.infea_model, s.infea_infty);
    L.add(L.BOTH, z.nq, s.trial, s.succ, s.fail, s.hu_word, s.exitflag, s.nwsr_qp, s.nwsr_lp, s.rounds);
}
}  // namespace rsqp_batch_units
