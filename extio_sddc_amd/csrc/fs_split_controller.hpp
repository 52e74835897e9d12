// fs_split_controller.hpp — the adaptive static frame split of the d = 0 kernel (ddc_fs.hip): the
// host-side controller that learns each workgroup's share of a launch's frames from the measured
// start and end times of the launches before it (plain C++, no HIP: tests/test_adaptive_split.py
// drives it on the CPU through sddc_fs_split_* of ddc_runtime.cpp).
//
// Why.  At full residency (grid = 4 x CUs) blockIdx lands on the same CU and CU slot in every
// launch, and a workgroup's end time repeats: of 7.8 us rms deviation from the launch's mean end,
// 7.4 us repeated over 12 launches and 2.5 us was noise (profiles/adaptive_split/before_repeat.txt:
// slot 6.9, XCD 2.2, place in the quarter 1.0, the individual workgroup 0.8 us rms).  The launch
// lasts until the last workgroup ends, and which slot, XCD or CU is slow is a property of the box,
// so the built-in slot weights (kFsSlotWeights) cannot be right everywhere.
//
// Model.  Workgroup w starts o[w] after the launch's first workgroup and takes c[w] per frame,
// both in units of the launch's mean time per frame (so the clock's state drops out).  A launch
// of ns frames gives workgroup w the largest n[w] with o[w] + n[w] c[w] <= T, T the smallest
// value for which the n[w] add up to ns: the integer split with the earliest last end
// (allocate()).  Each n[w] stays within +-kClamp of the built-in split's, so nothing a disturbed
// measurement (another process on the GPU, a profiler, overlapping launches) teaches can produce a
// pathological split.  A measurement moves c[w] by a damped, bounded multiplicative step towards
// the observed cost (update()): at most a factor 1 + kEta (kStep - 1) per launch.
// Cold start (no measurement yet, or another batch size) is the built-in split itself.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "fs_shares.h"

namespace sddc {

// the built-in slot-weighted split: ddc_queue.hpp slot_split, restated for the host
inline int fs_slot_split_host(int ns, int G, int v, unsigned slotw)
{
    if (slotw == 0u || (G & 3)) return (int)(((long long)ns * v) / G);
    const int Q = G >> 2, q = v / Q, i = v - q * Q;
    long long sw = 0, tot = 0;
    for (int k = 0; k < 4; k++) {
        const int wk = (int)((slotw >> (8 * k)) & 0xffu);
        tot += (long long)Q * wk;
        if (k < q) sw += (long long)Q * wk;
        else if (k == q) sw += (long long)i * wk;
    }
    return (int)(((long long)ns * sw) / tot);
}

class FsSplitController {
public:
    static constexpr double kEta = 0.25;     // damping of a step
    static constexpr double kStep = 1.25;    // bound of one observation's cost ratio (and its inverse)
    static constexpr double kClamp = 0.25;   // frames of a workgroup: within this of the built-in split's
    static constexpr double kCostSpan = 2.0; // c[w] stays within this factor of the cold-start cost
    static constexpr double kMaxOffset = 8.0;   // start offsets above this many frame times are cut

    void reset(int G, unsigned slotw)
    {
        G_ = G;
        slotw_ = slotw;
        measured_ = 0;
        ns_ = 0;
        c0_.assign((size_t)G, 1.0);
        if (slotw != 0u && !(G & 3)) {
            double sum = 0.0;
            for (int k = 0; k < 4; k++) sum += (double)((slotw >> (8 * k)) & 0xffu);
            for (int w = 0; w < G; w++) c0_[(size_t)w] = sum / 4.0 / (double)((slotw >> (8 * (w / (G >> 2)))) & 0xffu);
        }
        c_ = c0_;
        o_.assign((size_t)G, 0.0);
        forced_.clear();
    }
    int groups() const { return G_; }
    unsigned slot_weights() const { return slotw_; }
    long measured() const { return measured_; }
    bool forced() const { return !forced_.empty(); }
    // warm: table() describes something other than the built-in split
    bool warm() const { return forced() || measured_ > 0; }
    const std::vector<double> &cost() const { return c_; }
    const std::vector<double> &offset() const { return o_; }

    // the batch size the state was learnt at: another one starts cold again (a workgroup's cost
    // per frame depends on how long its neighbours stay resident)
    void set_frames(int ns)
    {
        if (ns != ns_ && measured_ > 0) {
            const std::vector<double> f = forced_;
            reset(G_, slotw_);
            forced_ = f;
        }
        ns_ = ns;
    }

    // a given table of relative shares (>= 0, not all zero), used as it is (no clamp) until
    // unload(): the tests' forced splits
    bool load(const float *shares, int n)
    {
        if (n != G_ || !shares) return false;
        double sum = 0.0;
        for (int w = 0; w < n; w++) {
            if (!(shares[w] >= 0.f) || !std::isfinite(shares[w])) return false;
            sum += shares[w];
        }
        if (!(sum > 0.0)) return false;
        forced_.resize((size_t)n);
        for (int w = 0; w < n; w++) forced_[(size_t)w] = shares[w] / sum;
        return true;
    }
    void unload() { forced_.clear(); }

    // frames per workgroup of a launch of ns frames
    void allocate(int ns, int *n) const
    {
        const int G = G_;
        if (forced()) {
            double cum = 0.0;
            long long prev = 0;
            for (int w = 0; w < G; w++) {
                cum += forced_[(size_t)w];
                long long A = w == G - 1 ? ns : (long long)std::floor(cum * ns + 0.5);
                A = std::min<long long>(std::max(A, prev), ns);
                n[w] = (int)(A - prev);
                prev = A;
            }
            return;
        }
        lo_.resize((size_t)G);
        hi_.resize((size_t)G);
        ic_.resize((size_t)G);
        double tmax = 0.0;
        for (int w = 0; w < G; w++) {
            const int base = fs_slot_split_host(ns, G, w + 1, slotw_) - fs_slot_split_host(ns, G, w, slotw_);
            lo_[(size_t)w] = (int)(base * (1.0 - kClamp));
            hi_[(size_t)w] = (int)std::ceil(base * (1.0 + kClamp));
            ic_[(size_t)w] = 1.0 / c_[(size_t)w];
            tmax = std::max(tmax, o_[(size_t)w] + (hi_[(size_t)w] + 1) * c_[(size_t)w]);
        }
        auto count = [&](double T, int *out) {
            long long tot = 0;
            for (int w = 0; w < G; w++) {
                const double x = (T - o_[(size_t)w]) * ic_[(size_t)w];
                int k = x > 0.0 ? (x < 2.0e9 ? (int)x : 2000000000) : 0;
                k = std::min(std::max(k, lo_[(size_t)w]), hi_[(size_t)w]);
                if (out) out[w] = k;
                tot += k;
            }
            return tot;
        };
        double a = 0.0, b = tmax;   // count(b) = sum hi >= ns
        for (int it = 0; it < 40; it++) {
            const double T = 0.5 * (a + b);
            if (count(T, nullptr) >= ns) b = T;
            else a = T;
        }
        long long extra = count(b, n) - ns;
        // several workgroups may cross a frame boundary at the same T: take the surplus back where
        // the end is latest (and, should the clamps have left a deficit, add where it is earliest)
        while (extra > 0) {
            int best = -1;
            double be = -1.0;
            for (int w = 0; w < G; w++) {
                const double e = o_[(size_t)w] + n[w] * c_[(size_t)w];
                if (n[w] > lo_[(size_t)w] && e > be) be = e, best = w;
            }
            if (best < 0) break;
            n[best]--;
            extra--;
        }
        while (extra < 0) {
            int best = -1;
            double be = 1e300;
            for (int w = 0; w < G; w++) {
                const double e = o_[(size_t)w] + (n[w] + 1) * c_[(size_t)w];
                if (n[w] < hi_[(size_t)w] && e < be) be = e, best = w;
            }
            if (best < 0) break;
            n[best]++;
            extra++;
        }
        // the clamps cannot hold ns (sum lo > ns or sum hi < ns: neither happens for a base split
        // that sums to ns): the last workgroup takes the difference
        if (extra != 0) n[G - 1] = (int)std::max<long long>(0, n[G - 1] - extra);
    }

    // the launch's table; n receives the frames per workgroup the table gives (what the kernel
    // computes: above 32768 frames the table's grid, fs_shares.h)
    void table(int ns, FsShares *t, int *n) const
    {
        const int G = G_;
        allocate(ns, n);
        long long A = 0;
        for (int w = 0; w < kFsShareMaxG / 2; w++) t->p[w] = 0u;
        for (int w = 0; w < G; w++) {
            fs_share_set(*t, w, fs_share_of(A, ns));
            A += n[w];
        }
        for (int w = 0; w < G; w++) n[w] = fs_share_start(ns, G, w + 1, *t) - fs_share_start(ns, G, w, *t);
    }

    // one launch's measurement: frames, start and end (ticks of one free-running 32-bit counter)
    // per workgroup.  false: rejected as a whole (nothing changes).
    bool update(const int *n, const uint32_t *start, const uint32_t *end)
    {
        const int G = G_;
        if (forced()) return false;
        double sum_d = 0.0;
        long long sum_n = 0;
        int32_t first = 0;
        for (int w = 0; w < G; w++) {
            const uint32_t d = end[w] - start[w];
            if (n[w] < 0 || d > 0x40000000u || (n[w] > 0 && d == 0u)) return false;   // (an empty range may take no tick)
            const int32_t rel = (int32_t)(start[w] - start[0]);
            first = std::min(first, rel);
            sum_d += n[w] > 0 ? (double)d : 0.0;
            sum_n += n[w];
        }
        if (sum_n <= 0 || !(sum_d > 0.0)) return false;
        const double m = sum_d / (double)sum_n;   // the launch's mean time per frame
        double norm = 0.0;
        for (int w = 0; w < G; w++) {
            double &c = c_[(size_t)w];
            if (n[w] > 0) {
                const double obs = (double)(end[w] - start[w]) / (n[w] * m);
                const double r = std::min(std::max(obs / c, 1.0 / kStep), kStep);
                c *= 1.0 + kEta * (r - 1.0);
            }
            const double so = std::min((double)((int32_t)(start[w] - start[0]) - first) / m, kMaxOffset);
            o_[(size_t)w] += kEta * (so - o_[(size_t)w]);
            norm += c / c0_[(size_t)w];
        }
        // only the costs' ratios matter: keep their scale at the cold start's, each within kCostSpan
        norm /= G;
        for (int w = 0; w < G; w++) {
            const double c0 = c0_[(size_t)w];
            c_[(size_t)w] = std::min(std::max(c_[(size_t)w] / norm, c0 / kCostSpan), c0 * kCostSpan);
        }
        measured_++;
        return true;
    }

private:
    int G_ = 0, ns_ = 0;
    unsigned slotw_ = 0u;
    long measured_ = 0;
    std::vector<double> c0_, c_, o_, forced_;
    mutable std::vector<int> lo_, hi_;
    mutable std::vector<double> ic_;
};

}  // namespace sddc
