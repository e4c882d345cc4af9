// String layer, part 2 of 7: single-block 0/1 flags and their trees (fused mode).
#include "strings.h"

#include <algorithm>
#include <cstring>
#include <set>

#include "strings_internal.h"

namespace fhs {

// ---------------------------------------------------------------------------------------------
// fused mode: single-block 0/1 flags, sums of up to 15 flags per PBS (the carry space holds 15),
// log_15-depth AND/OR trees.  Decrypts identically to the as-written mode.
// ---------------------------------------------------------------------------------------------
Ref sum_refs(Engine *e, const Ref *r, size_t n) {
    // any length: the callers bound the VALUE of the sum (15 flags, one-hot picks, noise budget), not the number of
    // terms -- trivial blocks carry no noise and fold into the constant, so a sum over a mostly plaintext string can be
    // long (first_index on 256 trivial windows: 64 blocks; found by tests/test_folded_strings.py)
    std::vector<Term> tt(n);
    for (size_t i = 0; i < n; i++) tt[i] = {1, r[i].id()};
    return Ref(e, e->lin(tt.data(), n, 0));
}

// Flags that are the SAME block (one bootstrap shared by several windows of a mostly plaintext string: the engine's
// common-subexpression table hands out one node) count once in an AND / OR -- summed, they would come back as ONE term
// with a coefficient of up to 15, i.e. 225 times the variance of a flag.
// "The same" is structural: a flag may be a linear form over a block (1 - bad of char_significant, 1 - same ...), a new
// node every time it is built, so two nodes are the same flag when they are the same block or the same constant + terms
// (a string that holds one ciphertext several times -- `repeat`, a caller's own FheString -- produces those).
// One canonical key per flag -- the block id, or for a linear form its constant and its sorted (block, coefficient)
// terms -- and an order-preserving de-duplication through a sorted set: O(n log n) in the number of flags (an and_tree
// over 4096 characters compares thousands; pairwise comparison with two sorted temporaries each was O(n^2) allocations
// on the host planning path).
using FlagKey = std::vector<int64_t>;
static FlagKey flag_key(const Engine *e, Bid a) {
    const BlockNode &x = e->node(a);
    if (x.kind != BlockNode::LIN) return {0, (int64_t)a};
    std::vector<std::pair<Bid, int64_t>> tt;
    tt.reserve(x.terms.size());
    for (const Term &t : x.terms) tt.emplace_back(t.blk, t.coef);
    std::sort(tt.begin(), tt.end());
    if (tt.size() == 1 && tt[0].second == 1 && x.konst == 0) return {0, (int64_t)tt[0].first};   // 1 * block: that block
    FlagKey k{1, (int64_t)x.konst};
    for (auto &t : tt) { k.push_back((int64_t)t.first); k.push_back(t.second); }
    return k;
}
void distinct_flags(const Engine *e, std::vector<Ref> &f) {
    if (f.size() < 2) return;
    std::set<FlagKey> seen;
    std::vector<Ref> out;
    out.reserve(f.size());
    for (Ref &x : f)
        if (seen.insert(flag_key(e, x.id())).second) out.push_back(x);
    f.swap(out);
}

Ref Strings::flag_not(const Ref &x) {
    const Ref one = trivial_block(e_, 1);
    return lin(e_, {{1, &one}, {-1, &x}});
}

// The flags of an AND (absorbing = 0) or an OR (absorbing = 1) without the trivial ones: a trivial 1 says nothing in an
// AND, a trivial 0 nothing in an OR.  false when a trivial flag decides: the result is the trivial `absorbing`.
bool Strings::drop_trivial(std::vector<Ref> &f, int absorbing) const {
    std::vector<Ref> kept;
    for (const Ref &x : f) {
        if (!e_->is_triv(x.id())) kept.push_back(x);
        else if ((int)(e_->triv_val(x.id()) & 1) == absorbing) return false;
    }
    f.swap(kept);
    return true;
}

// and_tree (absorbing = 0: a group of n flags is all set iff its sum is n) and or_tree (absorbing = 1: iff it is not 0)
Ref Strings::flag_tree(std::vector<Ref> cur, int absorbing) {
    if (!drop_trivial(cur, absorbing)) return trivial_block(e_, absorbing);
    if (cur.empty()) return trivial_block(e_, 1 - absorbing);
    while (cur.size() > 1) {
        distinct_flags(e_, cur);
        if (cur.size() == 1) break;
        std::vector<Ref> nxt;
        for (size_t i = 0; i < cur.size(); i += 15) {
            const size_t n = std::min<size_t>(15, cur.size() - i);
            if (n == 1) nxt.push_back(cur[i]);
            else nxt.push_back(pbs(sum_refs(e_, &cur[i], n), absorbing ? LUT_NZ : lut_is_k((int)n)));
        }
        cur.swap(nxt);
    }
    return cur[0];
}

// OR of flags of which AT MOST ONE is set.  Their sum never exceeds 1, so it is the noise budget, not the 4-bit message
// space, that limits a group: up to FHS_NOISE_BUDGET_SUM_C2 fresh flags per refreshing bootstrap instead of 15, and the
// last few partial sums (sum c^2 <= 4) are handed back as a linear combination without a bootstrap of their own.
// 4097 flags: 65 + 2 bootstraps in 2 levels instead of 274 + 19 + 2 + 1 in 4 (the verdict of a 4096-character `le`).
Ref Strings::onehot_or(std::vector<Ref> cur) {
    if (!drop_trivial(cur, 1)) return trivial_block(e_, 1);
    if (cur.empty()) return trivial_block(e_, 0);
    for (;;) {
        if (cur.size() == 1) return cur[0];
        int64_t total = 0;
        for (const Ref &x : cur) total += e_->sum_c2(x.id());
        if (total <= 4) {
            Term tt[4];
            for (size_t i = 0; i < cur.size(); i++) tt[i] = {1, cur[i].id()};
            return Ref(e_, e_->lin(tt, cur.size(), 0));
        }
        std::vector<Ref> nxt;
        Term tt[FHS_NOISE_BUDGET_SUM_C2];
        size_t m = 0;
        int64_t c2 = 0;
        auto close = [&] {
            if (m == 1) nxt.push_back(Ref(e_, (e_->retain(tt[0].blk), tt[0].blk)));
            else if (m > 1) nxt.push_back(pbs(Ref(e_, e_->lin(tt, m, 0)), LUT_NZ));
            m = 0;
            c2 = 0;
        };
        for (const Ref &x : cur) {
            const int64_t w = std::max<int64_t>(1, e_->sum_c2(x.id()));
            if (c2 + w > FHS_NOISE_BUDGET_SUM_C2 || m == (size_t)FHS_NOISE_BUDGET_SUM_C2) close();
            tt[m++] = {1, x.id()};
            c2 += w;
        }
        close();
        cur.swap(nxt);
    }
}

FChar Strings::flags_or(const FStr &flags) {
    std::vector<Ref> f;
    for (const FChar &c : flags) f.push_back(c.b[0]);
    return ch_flag(e_, or_tree(f));
}
FChar Strings::flags_and(const FStr &flags) {
    std::vector<Ref> f;
    for (const FChar &c : flags) f.push_back(c.b[0]);
    return ch_flag(e_, and_tree(f));
}

// The input of a bootstrap as sum coef[k] * blk[k] over four char blocks (clean 2-bit digits), which may be short sums of
// bootstrap outputs (a select is SEL_T + SEL_F, a case shift adds 2 x flag, ...).  The noise is measured on the
// FLATTENED combination: blocks that share bootstrap outputs (common subexpressions; sel / covered of f_replace_expand
// stand in all four digits of a selected character) add their coefficients BEFORE squaring -- per-block sums under-count
// that (120 for replace with an 8-character `from`).  If it would carry more than the noise budget, the
// blocks that are sums are refreshed in place (LUT_MSG keeps a clean digit) and the combination is built again.
Ref Strings::lin_in_budget(Ref *const blk[4], const int64_t coef[4]) {
    auto build = [&] { return lin(e_, {{coef[0], blk[0]}, {coef[1], blk[1]}, {coef[2], blk[2]}, {coef[3], blk[3]}}); };
    Ref d = build();
    if (e_->sum_c2(d.id()) <= FHS_NOISE_BUDGET_SUM_C2) return d;
    for (int k = 0; k < 4; k++)
        if (e_->sum_c2(blk[k]->id()) > 1) *blk[k] = pbs(*blk[k], LUT_MSG);
    return build();
}

// Equality of two chars as the AND of 2 flags: nibbles (x0 + 4 x1, x2 + 4 x3) are packed linearly,
// and (a_nib - b_nib) in [-15, 15] is tested with the `is0` LUT.  That LUT is safe under the
// padding-bit rule: a negative difference lands on 32-k, whose PBS value is -f(16-k) = -0 = 0.
std::vector<Ref> Strings::block_eq_flags(const FChar &a_in, const FChar &b_in) {
    static const int64_t coef[4] = {1, 4, -1, -4};
    FChar a = a_in, b = b_in;
    std::vector<Ref> f;
    for (int h = 0; h < 2; h++) {
        Ref *const blk[4] = {&a.b[2 * h], &a.b[2 * h + 1], &b.b[2 * h], &b.b[2 * h + 1]};
        f.push_back(pbs(lin_in_budget(blk, coef), LUT_IS0));
    }
    return f;
}

// The two nibble flags of [c == byte]; with both_cases, of [c == byte or c == byte ^ 0x20] for an ASCII letter: the cases
// share the low nibble and have high nibbles 4 / 6 or 5 / 7, so the high-nibble flag is the sum of two extractions of
// one rotation (the same test, the other row), charged as fully correlated by lin_c2 (4).
std::vector<Ref> Strings::byte_eq_flags(const FChar &c, uint8_t byte, bool both_cases) {
    std::vector<Ref> a = block_eq_flags(c, t(byte));
    if (both_cases) {
        const std::vector<Ref> b = block_eq_flags(c, t(byte ^ 0x20));
        a[1] = lin(e_, {{1, &a[1]}, {1, &b[1]}});
    }
    return a;
}

Ref Strings::window_match(const FStr &s, size_t at, const FStr &pat) {
    std::vector<Ref> f;
    for (size_t j = 0; j < pat.size(); j++)
        for (Ref &x : block_eq_flags(s[at + j], pat[j])) f.push_back(x);
    return and_tree(f);
}

FChar Strings::f_contains(const FStr &s, const FStr &needle) {
    if (needle.empty()) return t(1);
    std::vector<Ref> w;
    for (size_t i = 0; i + needle.size() <= s.size(); i++) w.push_back(window_match(s, i, needle));
    return ch_flag(e_, or_tree(w));
}

// exclusive prefix OR of flags in log_15 depth: p[i] = OR_{k<i} f[k]
std::vector<Ref> Strings::prefix_or(const std::vector<Ref> &f) {
    const size_t n = f.size();
    std::vector<Ref> p(n);
    if (n == 0) return p;
    const size_t nchunks = (n + 14) / 15;
    std::vector<Ref> q, any;                 // q: exclusive prefix OR over whole chunks, any: the chunks' totals
    if (nchunks > 1) {
        any.resize(nchunks - 1);             // the last chunk's total is never needed
        for (size_t j = 0; j + 1 < nchunks; j++) {
            std::vector<Ref> grp(f.begin() + 15 * j, f.begin() + 15 * j + 15);
            distinct_flags(e_, grp);                              // an OR: a flag that occurs twice counts once (noise)
            any[j] = pbs(sum_refs(e_, grp.data(), grp.size()), LUT_NZ);
        }
        any.push_back(trivial_block(e_, 0));
        q = prefix_or(any);
    } else {
        q.push_back(trivial_block(e_, 0));
    }
    auto depth = [&](const Ref &r) { return e_->node(r.id()).level; };
    for (size_t i = 0; i < n; i++) {
        const size_t j = i / 15, k = i % 15;
        std::vector<Ref> terms(f.begin() + 15 * j, f.begin() + 15 * j + k);
        // the 16th chunk's prefix is the OR of 16 totals, one level deeper than its neighbours': the previous chunk's
        // prefix and total say the same one level earlier (find on 256 characters ends one launch sooner)
        if (j >= 1 && k >= 1 && k <= 13 && depth(q[j]) > std::max(depth(q[j - 1]), depth(any[j - 1]))) {
            terms.push_back(q[j - 1]);
            terms.push_back(any[j - 1]);
            distinct_flags(e_, terms);
            p[i] = pbs(sum_refs(e_, terms.data(), terms.size()), LUT_NZ);
            continue;
        }
        const bool q0 = e_->is_triv(q[j].id()) && e_->triv_val(q[j].id()) == 0;
        if (k == 0) { p[i] = q[j]; continue; }               // nothing of this chunk yet: the flag itself, no bootstrap
        if (k == 1 && q0) { p[i] = f[15 * j]; continue; }    // OR of one 0/1 flag
        terms.push_back(q[j]);
        distinct_flags(e_, terms);               // an OR: the same flag twice counts once (<= 14 + 1 terms)
        p[i] = pbs(sum_refs(e_, terms.data(), terms.size()), LUT_NZ);   // folds to a constant when everything is trivial
    }
    return p;
}

std::vector<Ref> Strings::suffix_or(const std::vector<Ref> &f) {
    std::vector<Ref> rev(f.rbegin(), f.rend());
    std::vector<Ref> p = prefix_or(rev);
    return std::vector<Ref>(p.rbegin(), p.rend());
}

// [c == 0] or [c != 0] in ONE bootstrap: the four base-4 digits are non-negative, so their sum (<= 12, inside the message
// space) is zero iff every digit is -- instead of two nibble tests and a combining bootstrap.  Digits that are sums of
// bootstrap outputs are refreshed first only if together they would leave the noise budget (lin_in_budget).
Ref Strings::char_zero_test(const FChar &c_in, bool want_zero) {
    static const int64_t coef[4] = {1, 1, 1, 1};
    FChar c = c_in;
    Ref *const blk[4] = {&c.b[0], &c.b[1], &c.b[2], &c.b[3]};
    return pbs(lin_in_budget(blk, coef), want_zero ? LUT_IS0 : LUT_NZ);
}

// NUL = 0x00, whitespace = 0x20, 0x09..0x0D (fheasciichar.rs:106-130): high nibble 0 with low nibble in
// {0, 9..13}, or high nibble 2 with low nibble 0 -- same 3-bootstrap shape as the case detector (row class of the high
// nibble, two range flags of the low nibble, the pick of the flag that belongs to the row)
Ref Strings::char_significant(const FChar &c) {
    Ref lo = lin(e_, {{1, &c.b[0]}, {4, &c.b[1]}});
    Ref hi = lin(e_, {{1, &c.b[2]}, {4, &c.b[3]}});
    Ref row = pbs(hi, LUT_HI_ROW02), cls = pbs(lo, LUT_LO_WSCLS);
    Ref bad = pbs(lin(e_, {{1, &row}, {4, &cls}}), LUT_CLS_PICK);
    return flag_not(bad);
}

// cond ? t : f with cond a clean single-block 0/1 flag (no scalar_ne needed)
FChar Strings::ite_flag(const Ref &flag_in, const FChar &tv_in, const FChar &fv_in) {
    FChar r;
    // the flag enters with weight 4: a flag that is itself a sum of several bootstrap outputs (one-hot cover sums,
    // 1 - x forms) is refreshed first when 16 x its sum c^2 would leave the noise budget
    Ref flag = flag_in;
    if (16 * e_->sum_c2(flag.id()) + 4 > FHS_NOISE_BUDGET_SUM_C2) flag = pbs(flag_in, LUT_NZ);
    const int64_t room = FHS_NOISE_BUDGET_SUM_C2 - 16 * e_->sum_c2(flag.id());
    FChar tv = tv_in, fv = fv_in;
    for (int i = 0; i < 4; i++) {                           // the selected digits enter with weight 1
        if (e_->sum_c2(tv.b[i].id()) > room) tv.b[i] = pbs(tv.b[i], LUT_MSG);
        if (e_->sum_c2(fv.b[i].id()) > room) fv.b[i] = pbs(fv.b[i], LUT_MSG);
    }
    for (int i = 0; i < 4; i++) {
        Ref a = pbs(lin(e_, {{4, &flag}, {1, &tv.b[i]}}), LUT_SEL_T);
        Ref b = pbs(lin(e_, {{4, &flag}, {1, &fv.b[i]}}), LUT_SEL_F);
        r.b[i] = lin(e_, {{1, &a}, {1, &b}});
    }
    return r;
}

}  // namespace fhs
