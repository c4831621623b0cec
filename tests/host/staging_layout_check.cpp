// staging_layout_check.cpp -- the staging block of the host-pointer batch calls (rsqp_batch_staging.h), checked on the host alone:
// no GPU, no HIP header. For each of the eight field tables and each shape (nq 1 and 13, with and without constraints, optional
// arrays absent and present) the offsets, the sizes and a round trip through two heap blocks of exactly words() doubles, the second
// standing in for the device. Every caller array is a heap block of exactly its documented size, so that AddressSanitizer sees an
// overrun on either side. Built and run by tests/test_staging_layout.py; exit status 0 = all held.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../restartsqp_amd/csrc/rsqp_batch_staging.h"

using namespace rsqp_batch_units;
using L = StagingLayout;

static int failures = 0;
static const char *where = "";
#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) { std::printf("FAIL %s: %s (line %d)\n", where, #cond, __LINE__); failures++; } \
    } while (0)

// the caller's arrays of one case: each a heap block of exactly its size, filled with values no other array holds
struct Arrays {
    struct One { std::unique_ptr<char[]> mem; std::vector<char> before; size_t bytes; };
    std::vector<One> all;
    int serial = 0;
    template <class T>
    T *make(size_t count, bool present = true) {
        if (!present) return nullptr;
        One a{std::unique_ptr<char[]>(new char[count * sizeof(T)]), {}, count * sizeof(T)};
        T *const p = reinterpret_cast<T *>(a.mem.get());
        serial++;
        for (size_t i = 0; i < count; i++) p[i] = (T)(1000 * serial + (int)i);
        a.before.assign(a.mem.get(), a.mem.get() + a.bytes);
        all.push_back(std::move(a));
        return p;
    }
    const One *find(const void *p) const {
        for (const One &a : all)
            if (a.mem.get() == p) return &a;
        return nullptr;
    }
};
static void *device_address(const L::Field &f) {
    void *p;
    std::memcpy(&p, f.ref, sizeof(p));
    return p;
}

// `lay` holds the declared table, its pointer fields still the caller's arrays
static void check(L &lay, const Arrays &arr, bool expect_tail) {
    CHECK(lay.ok());
    const size_t words = lay.words(), tail = lay.tail(), D = sizeof(double);
    size_t end = 0, sum = 0;
    bool down_seen = false;
    for (int k = 0; k < lay.count(); k++) {
        const L::Field &f = lay.field(k);
        CHECK(f.off >= end);                                     // disjoint and in declaration order
        CHECK(f.off - end < D);                                  // (nothing but the padding of an int run between two fields)
        CHECK(f.off % (f.is_int ? sizeof(int) : D) == 0);        // every double field on 8 bytes
        end = f.off + f.bytes;
        sum = ((f.is_int && (f.dir == L::UP || down_seen)) ? sum : (sum + D - 1) / D * D) + f.bytes;      // (the tail starts a word)
        if (f.dir != L::UP) { CHECK(f.off >= tail * D); down_seen = true; }
        else { CHECK(!down_seen); CHECK(f.off + f.bytes <= tail * D); }
        if (f.host) {                                            // the table's size of an array is the documented one
            const Arrays::One *a = arr.find(f.host);
            CHECK(a && a->bytes == f.bytes);
        }
    }
    CHECK(words * D == (end + D - 1) / D * D);
    CHECK(words * D == (sum + D - 1) / D * D);                   // words: the sum of the fields, int runs rounded up
    CHECK(tail <= words && lay.up_words() <= words);
    CHECK(expect_tail == (tail < words));

    // the round trip: host block -> "device" block (what goes up) -> the "device" writes -> tail back -> the caller's arrays
    std::unique_ptr<double[]> host(new double[words]), dev(new double[words]);
    std::memset(dev.get(), 0xA5, words * D);
    lay.pack(host.get());
    std::memcpy(dev.get(), host.get(), lay.up_words() * D);
    std::vector<void *> hosts;
    for (int k = 0; k < lay.count(); k++) hosts.push_back(lay.field(k).host);
    lay.address(dev.get());
    for (int k = 0; k < lay.count(); k++) {
        const L::Field &f = lay.field(k);
        char *const d = static_cast<char *>(device_address(f));
        CHECK(f.host == hosts[k]);
        if (!f.host) { CHECK(d == nullptr); continue; }          // a null array: a null device address
        CHECK(d == reinterpret_cast<char *>(dev.get()) + f.off);
        if (f.dir != L::DOWN) CHECK(std::memcmp(d, f.host, f.bytes) == 0);      // what went up is the caller's
        if (f.dir == L::UP) continue;
        // the device writes the first half of a both-way field (the rest belongs to members that sit out), all of a down field
        const size_t wr = f.dir == L::BOTH ? f.bytes / 2 : f.bytes;
        for (size_t i = 0; i < wr; i++) d[i] = (char)(37 * k + 11 * i + 1);
    }
    std::memcpy(host.get() + tail, dev.get() + tail, (words - tail) * D);
    lay.unpack(host.get());
    for (int k = 0; k < lay.count(); k++) {
        const L::Field &f = lay.field(k);
        if (!f.host) continue;
        const Arrays::One *a = arr.find(f.host);
        if (!a) continue;
        const char *const now = a->mem.get();
        if (f.dir == L::UP) { CHECK(std::memcmp(now, a->before.data(), a->bytes) == 0); continue; }   // untouched
        const size_t wr = f.dir == L::BOTH ? f.bytes / 2 : f.bytes;
        bool same = true;
        for (size_t i = 0; i < wr; i++) same = same && now[i] == (char)(37 * k + 11 * i + 1);
        CHECK(same);                                             // exactly what the device wrote
        CHECK(std::memcmp(now + wr, a->before.data() + wr, f.bytes - wr) == 0);     // the rest as it went up
    }
}

static void one_shape(size_t nq, bool constraints, bool optional) {
    // sN, sC: odd and unlike nq and each other, so that a table that names the wrong count fails the size check
    const StageSizes z{nq, 3 * nq + 2, constraints ? 2 * nq + 1 : 0};
    const bool C = constraints, O = optional;
    static char label[96];
    std::snprintf(label, sizeof(label), "nq=%zu sC=%zu optional=%d", z.nq, z.sC, (int)O);
    where = label;
    {   // rsqp_batch_handler_update
        Arrays m; L lay;
        rsqp_handler_iterate it{m.make<int>(z.nq), m.make<double>(z.nq), m.make<double>(z.nq), m.make<double>(z.sN),
                                m.make<double>(z.sN, O), m.make<double>(z.sC, C)};
        stage_iterate(lay, it, z);
        CHECK(lay.count() == 6);
        check(lay, m, false);
    }
    {   // rsqp_batch_handler_get_step
        Arrays m; L lay;
        double *p = m.make<double>(z.sN, O), *lam_c = m.make<double>(z.sC, O && C), *lam_x = m.make<double>(z.sN, O),
               *infea_model = m.make<double>(z.nq, O), *norm_p = m.make<double>(z.nq);
        stage_step(lay, p, lam_c, lam_x, infea_model, norm_p, z);
        CHECK(lay.count() == 5 && lay.tail() == 0 && lay.up_words() == 0);
        check(lay, m, true);
    }
    {   // rsqp_batch_handler_set_matrices: an array that is not given takes no room
        Arrays m; L lay;
        const size_t nJ = O ? 4 * nq + 1 : 0, nH = 2 * nq + 1;
        const int *what = m.make<int>(z.nq);
        const double *jac = m.make<double>(nJ, O), *hess = m.make<double>(nH);
        stage_matrices(lay, what, jac, hess, z.nq, nJ, nH);
        CHECK(lay.count() == 3 && lay.words() == (z.nq + 1) / 2 + nJ + nH);
        check(lay, m, false);
    }
    {   // rsqp_batch_handler_infeasibility
        Arrays m; L lay;
        const double *c = m.make<double>(z.sC, C);
        double *infea = m.make<double>(z.nq);
        stage_infeasibility(lay, c, infea, z);
        CHECK(lay.count() == 2 && lay.up_words() == z.sC && lay.tail() == z.sC);
        check(lay, m, true);
    }
    {   // rsqp_batch_handler_ratio_test
        Arrays m; L lay;
        rsqp_nlp_trial t{m.make<int>(z.nq), m.make<double>(z.nq), m.make<double>(z.nq), m.make<double>(z.sC, C), m.make<double>(z.sN),
                         m.make<double>(z.sC, C), m.make<double>(z.nq), m.make<double>(z.nq), m.make<double>(z.nq),
                         m.make<double>(z.nq, O), m.make<double>(z.nq, O), m.make<double>(z.nq, O), m.make<int>(z.nq, O),
                         m.make<int>(z.nq, O), m.make<int>(z.nq, O), m.make<int>(z.nq, O)};
        stage_trial(lay, t, z);
        CHECK(lay.count() == 16);
        check(lay, m, true);
    }
    {   // rsqp_batch_handler_check_optimality
        Arrays m; L lay;
        rsqp_nlp_point pt{m.make<int>(z.nq), m.make<double>(z.sN), m.make<double>(z.sN), m.make<double>(z.sC, C), m.make<double>(z.nq)};
        rsqp_optimality_status *out = reinterpret_cast<rsqp_optimality_status *>(m.make<double>(5 * z.nq, O));
        int *verdict = m.make<int>(z.nq, O);
        stage_point(lay, pt, out, verdict, z);
        CHECK(lay.count() == 7);
        check(lay, m, true);
    }
    {   // rsqp_batch_handler_update_penalty
        Arrays m; L lay;
        rsqp_penalty_state s{m.make<int>(z.nq), m.make<double>(z.nq), m.make<double>(z.nq), m.make<double>(z.sN), m.make<double>(z.sC, C),
                             m.make<double>(z.nq), m.make<double>(z.nq), m.make<int>(z.nq), m.make<int>(z.nq), m.make<int>(z.nq),
                             m.make<double>(z.nq, O), m.make<double>(z.nq, O), m.make<int>(z.nq, O), m.make<int>(z.nq, O),
                             m.make<int>(z.nq, O), m.make<int>(z.nq, O), m.make<int>(z.nq, O)};
        stage_penalty(lay, s, z);
        CHECK(lay.count() == 17);
        check(lay, m, true);
    }
    {   // rsqp_batch_handler_soc_begin / _soc_end: the 22 fields
        Arrays m; L lay;
        rsqp_soc_trial t{m.make<int>(z.nq), m.make<double>(z.nq), m.make<double>(z.nq), m.make<double>(z.sC, C), m.make<double>(z.sN),
                         m.make<double>(z.sC, C), m.make<double>(z.nq), m.make<double>(z.nq), m.make<double>(z.nq),
                         m.make<double>(z.nq, O), m.make<double>(z.nq, O), m.make<double>(z.nq, O), m.make<int>(z.nq, O),
                         m.make<int>(z.nq, O), m.make<int>(z.nq, O), m.make<int>(z.nq, O), m.make<double>(z.sN, O),
                         m.make<double>(z.nq, O), m.make<double>(z.sN), m.make<int>(z.nq), m.make<double>(z.nq, O), m.make<int>(z.nq, O)};
        stage_trial(lay, t, z);
        CHECK(lay.count() == 22);
        check(lay, m, true);
    }
}

int main() {
    for (size_t nq : {(size_t)1, (size_t)13})
        for (int constraints = 0; constraints < 2; constraints++)
            for (int optional = 0; optional < 2; optional++) one_shape(nq, constraints != 0, optional != 0);

    where = "the rules of the table";
    {   // one field more than the table holds is refused, not written
        L lay;
        double *p[L::CAP + 1] = {};
        for (int k = 0; k < L::CAP; k++) lay.add(L::BOTH, 1, p[k]);
        CHECK(lay.ok() && lay.count() == L::CAP);
        const size_t words = lay.words();
        lay.add(L::BOTH, 1, p[L::CAP]);
        CHECK(!lay.ok() && lay.count() == L::CAP && lay.words() == words);
    }
    {   // what comes down is one tail: an up-only field behind it is refused
        L lay;
        double *a = nullptr, *b = nullptr;
        const double *c = nullptr;
        lay.add(L::UP, 2, c);
        lay.add(L::BOTH, 2, a);
        lay.add(L::DOWN, 2, b);
        CHECK(lay.ok() && lay.count() == 3 && lay.tail() == 2 && lay.up_words() == 4 && lay.words() == 6);
        lay.add(L::UP, 2, c);
        CHECK(!lay.ok() && lay.count() == 3 && lay.words() == 6);
    }
    {   // the tail starts on a double word even behind half a word of ints
        L lay;
        const int *u = nullptr;
        int *d = nullptr;
        lay.add(L::UP, 3, u);
        lay.add(L::DOWN, 3, d);
        CHECK(lay.ok() && lay.tail() == 2 && lay.field(1).off == 16 && lay.words() == 4 && lay.up_words() == 2);
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("staging layout: all checks held\n");
    return 0;
}
