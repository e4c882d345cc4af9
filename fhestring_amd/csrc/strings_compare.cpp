// String layer, part 4 of 7: fused comparisons, case, trim and oblivious compaction.
#include "strings.h"

#include <algorithm>
#include <cstring>
#include <set>

#include "strings_internal.h"

namespace fhs {

// eq(to_lower(a), to_lower(b)) without folding either string: two characters are equal ignoring case iff their low
// nibbles are equal and their high nibbles are equal, or differ in the case bit 0x20 only with both characters letters
// (top two bits 01, and the low nibble in 1..15 on the rows 0x4_ / 0x6_, in 0..10 on the rows 0x5_ / 0x7_: with equal
// low nibbles one range test serves both).  6 bootstraps per position in 3 levels instead of 12 (case flags and folds
// of both strings, then the nibble tests); the length condition of eq is the tail test of f_eq (NUL has no case).
FChar Strings::f_eq_ignore_case(const FStr &a, const FStr &b) {
    std::vector<Ref> f;
    const size_t common = std::min(a.size(), b.size());
    auto clean = [&](FChar c) {                              // operands that are sums of bootstrap outputs (a select,
        for (int k = 0; k < 4; k++)                          // a case shift) are refreshed: the packings below weigh
            if (e_->sum_c2(c.b[k].id()) > 1) c.b[k] = pbs(c.b[k], LUT_MSG);   // them with up to 4
        return c;
    };
    for (size_t i = 0; i < common; i++) {
        const FChar x = clean(a[i]), y = clean(b[i]);
        Ref e_lo = pbs(lin(e_, {{1, &x.b[0]}, {4, &x.b[1]}, {-1, &y.b[0]}, {-4, &y.b[1]}}), LUT_IS0);
        Ref b3 = pbs(lin(e_, {{1, &x.b[3]}, {4, &y.b[3]}}), LUT_EQIC_B3);
        Ref z = pbs(lin(e_, {{1, &x.b[2]}, {4, &y.b[2]}}), LUT_EQIC_Z);
        Ref lo = pbs(lin(e_, {{1, &x.b[0]}, {4, &x.b[1]}}), LUT_EQIC_LO);
        Ref s1 = pbs(lin(e_, {{1, &z}, {4, &lo}}), LUT_EQIC_S1);
        // the three partial verdicts as one sum without collisions between a passing and a failing combination:
        // passing (B3, S1, E_lo) = (1, 1, 1), (2, 1, 1), (2, 2, 1) -> 11, 12, 15; sum c^2 = 59
        f.push_back(pbs(lin(e_, {{1, &b3}, {3, &s1}, {7, &e_lo}}), LUT_EQIC_FIN));
    }
    const FStr &longer = a.size() > b.size() ? a : b;
    for (size_t i = common; i < longer.size(); i++) f.push_back(char_zero_test(longer[i], true));
    return ch_flag(e_, and_tree(f));
}

// Lexicographic comparison (mod.rs:1470-1541) as a tree of three-state values.  A leaf is the sign of one nibble
// difference (a0 + 4 a1 - b0 - 4 b1 in [-15, 15] through the padding bit: -1 / 0 / 1), most significant first: position 0
// before position 1, the high nibble before the low one, a character one buffer does not have counts as NUL.  Three
// states reduce to one with sign(4 s1 + 2 s2 + s3) -- the first non-zero state decides, sum c^2 = 21 -- so the order of
// 2 n nibbles is known after 1 + log3(2 n) levels and ~3 n bootstraps.  (Rounds 1-2: per pair two signs, `lt` and `==`
// look-ups, a prefix OR over the `differs` flags, one pick per position and an OR over the picks: ~6 n bootstraps.)
// The reference decides by len(a) vs len(b) (numbers of non-zero characters) when no common position differs; with every
// common position equal those differ exactly by the non-zero characters in the longer buffer's tail, which is what the
// tail leaves (tail character against NUL) say.
std::vector<Ref> Strings::cmp_leaves(const FStr &a, const FStr &b) {
    const size_t n = std::max(a.size(), b.size());
    std::vector<Ref> st;
    st.reserve(2 * n);
    for (size_t i = 0; i < n; i++) {
        FChar ca = i < a.size() ? a[i] : t(0), cb = i < b.size() ? b[i] : t(0);
        for (int p = 1; p >= 0; p--) {
            Ref *blk[4] = {&ca.b[2 * p], &ca.b[2 * p + 1], &cb.b[2 * p], &cb.b[2 * p + 1]};
            Ref d = lin(e_, {{1, blk[0]}, {4, blk[1]}, {-1, blk[2]}, {-4, blk[3]}});
            if (e_->sum_c2(d.id()) > FHS_NOISE_BUDGET_SUM_C2) {  // operands that are sums of bootstrap outputs: refresh
                for (int k = 0; k < 4; k++)
                    if (e_->sum_c2(blk[k]->id()) > 1) *blk[k] = pbs(*blk[k], LUT_MSG);
                d = lin(e_, {{1, blk[0]}, {4, blk[1]}, {-1, blk[2]}, {-4, blk[3]}});
            }
            st.push_back(pbs(d, LUT_SIGN));
        }
    }
    return st;
}

Ref Strings::cmp_root_sum(std::vector<Ref> st) {
    while (st.size() > 3) {
        std::vector<Ref> nx;
        nx.reserve(st.size() / 3 + 1);
        for (size_t i = 0; i < st.size(); i += 3) {
            const size_t k = std::min<size_t>(3, st.size() - i);
            if (k == 1) nx.push_back(st[i]);
            else if (k == 2) nx.push_back(pbs(lin(e_, {{2, &st[i]}, {1, &st[i + 1]}}), LUT_SIGN));
            else nx.push_back(pbs(lin(e_, {{4, &st[i]}, {2, &st[i + 1]}, {1, &st[i + 2]}}), LUT_SIGN));
        }
        st.swap(nx);
    }
    if (st.size() == 3) return lin(e_, {{4, &st[0]}, {2, &st[1]}, {1, &st[2]}}, 8);
    if (st.size() == 2) return lin(e_, {{2, &st[0]}, {1, &st[1]}}, 8);
    if (st.size() == 1) return lin(e_, {{1, &st[0]}}, 8);
    return trivial_block(e_, 8);
}

FChar Strings::f_comparison(const FStr &a, const FStr &b, int cmp) {
    static const int root[4] = {LUT_LT8, LUT_LE8, LUT_GT8, LUT_GE8};
    return ch_flag(e_, pbs(cmp_root_sum(cmp_leaves(a, b)), root[cmp & 3]));   // two empty buffers: 8 = equal (:1490-1494)
}

// The positional half of the comparison on two equally long slices: (any position differs, verdict at the FIRST
// differing position; 0 when none differs).  Multi-GPU position sharding combines these per-range partials: the
// first range that differs decides (fhestring_amd/parallel.py ShardedCmp).
void Strings::f_cmp_partial(const FStr &a, const FStr &b, int cmp, FChar *any_diff_out, FChar *verdict_out) {
    const size_t n = std::min(a.size(), b.size());
    if (n == 0) {
        *any_diff_out = t(0);
        *verdict_out = t(0);
        return;
    }
    FStr ca(a.begin(), a.begin() + n), cb(b.begin(), b.begin() + n);
    Ref v = cmp_root_sum(cmp_leaves(ca, cb));
    Ref same = pbs(v, LUT_IS8);
    *verdict_out = ch_flag(e_, pbs(v, (cmp == 0 || cmp == 1) ? LUT_LT8 : LUT_GT8));
    *any_diff_out = ch_flag(e_, flag_not(same));
}

// Combines per-range partials of f_cmp_partial (ranges in string order): the first range that differs decides;
// if none differs the result is `tie` (1 for le / ge, 0 for lt / gt: equal buffers are equal strings).
FChar Strings::flags_first_decides(const FStr &any_diff, const FStr &verdict, int tie) {
    const size_t n = std::min(any_diff.size(), verdict.size());
    if (n == 0) return t(tie ? 1 : 0);
    std::vector<Ref> d(n), pick(n);
    for (size_t r = 0; r < n; r++) d[r] = any_diff[r].b[0];
    std::vector<Ref> before = prefix_or(d);                  // exclusive: some earlier range differs
    for (size_t r = 0; r < n; r++) pick[r] = pbs(lin(e_, {{2, &verdict[r].b[0]}, {1, &before[r]}}), LUT_IS2);
    Ref ret = onehot_or(pick);                               // at most one pick is set
    if (tie) {                                               // ret = 1 implies a difference: the sum stays in {0, 1}
        Ref one = trivial_block(e_, 1), any = or_tree(d);
        ret = lin(e_, {{1, &ret}, {1, &one}, {-1, &any}});
    }
    return ch_flag(e_, ret);
}

// ends_with (mod.rs:241-288) re-associated: the result is the match flag of the LAST window that
// contains no NUL ("use the last result that has not encountered padding", :281-286), 0 if none.
FChar Strings::f_ends_with(const FStr &s, const FStr &needle, std::vector<Ref> *pick_out) {
    const size_t W = s.size() - needle.size() + 1;
    std::vector<Ref> nzc(s.size());
    for (size_t k = 0; k < s.size(); k++) nzc[k] = char_zero_test(s[k], false);
    std::vector<Ref> valid(W), match(W);
    for (size_t i = 0; i < W; i++) {
        std::vector<Ref> v(nzc.begin() + i, nzc.begin() + i + needle.size());
        valid[i] = and_tree(v);
        match[i] = needle.empty() ? trivial_block(e_, 1) : window_match(s, i, needle);
    }
    std::vector<Ref> after = suffix_or(valid);
    std::vector<Ref> pick(W);
    for (size_t i = 0; i < W; i++)                           // match & valid & !after
        pick[i] = pbs(lin(e_, {{1, &match[i]}, {1, &valid[i]}, {4, &after[i]}}), LUT_IS2);
    Ref res = or_tree(pick);
    if (pick_out) *pick_out = pick;
    return ch_flag(e_, res);
}

// trim_end / the marking half of trim_start (trim.rs:36-57, 86-115): a char survives iff some
// non-NUL, non-whitespace char sits at or after it (from_end) / at or before it
FStr Strings::f_trim(const FStr &s, bool from_end) {
    const size_t n = s.size();
    std::vector<Ref> sig(n);
    for (size_t i = 0; i < n; i++) sig[i] = char_significant(s[i]);
    std::vector<Ref> other = from_end ? suffix_or(sig) : prefix_or(sig);
    const FChar zero = t(0);
    FStr r(n);
    for (size_t i = 0; i < n; i++) {
        Ref stop = pbs(lin(e_, {{1, &sig[i]}, {1, &other[i]}}), LUT_NZ);   // inclusive OR
        r[i] = ite_flag(stop, s[i], zero);
    }
    return r;
}

// sum of up to 4 base-4 numbers (+ carry) with a sequential carry chain; result has `digits` digits
Strings::Num Strings::num_add(const std::vector<const Num *> &ops, size_t digits) {
    Num r(digits);
    Ref carry;
    for (size_t d = 0; d < digits; d++) {
        Term tt[8];
        size_t k = 0;
        for (const Num *o : ops)
            if (d < o->size()) tt[k++] = {1, (*o)[d].id()};
        if (carry) tt[k++] = {1, carry.id()};
        Ref sm(e_, e_->lin(tt, k, 0));                      // <= 4*3 + 3
        r[d] = pbs(sm, LUT_MSG);
        if (d + 1 < digits) carry = pbs(sm, LUT_CARRY);
    }
    return r;
}

// exclusive prefix sums of numbers, 4-ary recursion (depth log4(n) x 2 adds)
std::vector<Strings::Num> Strings::num_exclusive_scan(const std::vector<Num> &x, size_t digits) {
    const size_t n = x.size();
    std::vector<Num> out(n);
    Num zero(digits);
    for (auto &d : zero) d = trivial_block(e_, 0);
    if (n == 0) return out;
    if (n == 1) { out[0] = zero; return out; }
    const size_t ng = (n + 3) / 4;
    std::vector<Num> local(n), totals(ng);
    for (size_t g = 0; g < ng; g++) {
        const size_t lo = 4 * g, hi = std::min(n, lo + 4);
        std::vector<const Num *> ops;
        for (size_t i = lo; i < hi; i++) {
            local[i] = ops.empty() ? zero : (ops.size() == 1 ? *ops[0] : num_add(ops, digits));
            ops.push_back(&x[i]);
        }
        totals[g] = ops.size() == 1 ? *ops[0] : num_add(ops, digits);
    }
    std::vector<Num> offs = num_exclusive_scan(totals, digits);
    for (size_t i = 0; i < n; i++) out[i] = num_add({&offs[i / 4], &local[i]}, digits);
    return out;
}

// The number of set flags among k <= 15 as a base-4 number (low digit, high digit, zeros): two look-ups on their sum.
// Flags that are ONE block (the same character twice in a string: `repeat`; NUL tests of identical neighbourhoods of a
// mostly plaintext string, shared by the common-subexpression table) come back from the sum as one term with their
// multiplicity as coefficient -- a count of k equal flags IS k times the flag -- and 9 of them already pass the noise
// budget (81 > 64).  Then the flags are counted in two halves and the halves added as numbers.
Strings::Num Strings::count_digits(const Ref *flags, size_t k, size_t D) {
    Ref sum = k ? sum_refs(e_, flags, k) : trivial_block(e_, 0);
    if (k > 1 && e_->sum_c2(sum.id()) > FHS_NOISE_BUDGET_SUM_C2) {
        Num a = count_digits(flags, k / 2, D), b = count_digits(flags + k / 2, k - k / 2, D);
        return num_add({&a, &b}, D);
    }
    Num v(D);
    for (size_t d = 0; d < D; d++) v[d] = d == 0 ? pbs(sum, LUT_MSG) : (d == 1 ? pbs(sum, LUT_CARRY) : trivial_block(e_, 0));
    return v;
}

// Exclusive prefix counts of 0/1 flags as base-4 numbers: chunks of 15 flags give a (low, high) digit pair each, an
// exclusive scan over the chunk totals (4-ary, log depth) and one add per position.
std::vector<Strings::Num> Strings::flag_prefix_counts(const std::vector<Ref> &z, size_t D) {
    const size_t n = z.size();
    std::vector<Num> out(n);
    if (n == 0) return out;
    const size_t nch = (n + 14) / 15;
    std::vector<Num> tot(nch);
    for (size_t j = 0; j < nch; j++) tot[j] = count_digits(&z[15 * j], std::min<size_t>(15, n - 15 * j), D);
    std::vector<Num> offs = num_exclusive_scan(tot, D);
    for (size_t i = 0; i < n; i++) {
        const size_t j = i / 15, k = i % 15;
        Num loc = count_digits(&z[15 * j], k, D);
        out[i] = num_add({&offs[j], &loc}, D);
    }
    return out;
}

// Oblivious order-preserving compaction: non-NUL characters move left by the number of NULs before
// them.  Shifts are prefix counts (base-4 numbers), routed LSB first through log2(n) conditional
// moves by 2^k -- collision-free for monotone compaction.  Same result as the reference's n-pass
// bubble (utils.rs:28-46) in O(n log n) PBS and O(log n) wide levels instead of O(n^2) / O(n).
// The not-yet-used part of every shift travels with its character as base-4 DIGITS, and the bit a stage needs is
// extracted from its digit where it is used (1 bootstrap).  A stage costs ONE bootstrap per block or digit: the part
// that moves is m = (bit ? x : 0), and what stays is x - m -- linear, exact (m is x or 0) -- so
//     next[p] = cur[p] - m[p] + m[p + 2^k].
// The blocks are sums of 1 + 2k bootstrap outputs by then (sum c^2 <= 23, the select's input 16 + 21), inside the noise
// budget; the result is refreshed once at the end.  101 bootstraps per position for n = 1025 instead of 209 (bits
// routed separately, stay and move selected separately).
FStr Strings::f_compact(const FStr &s) {
    const size_t n = s.size();
    if (n <= 1) return s;
    int K = 0;
    while (((size_t)1 << K) < n) K++;                       // shifts are < n
    const size_t D = (size_t)(K + 1) / 2;
    const FChar zero = t(0);
    std::vector<Ref> z(n);
    for (size_t i = 0; i < n; i++) z[i] = char_zero_test(s[i], true);   // is-NUL flag: one bootstrap on the digit sum
    // per-position shift = number of NULs before it; NUL positions get shift 0 (they stay and contribute zeros)
    std::vector<Num> shifts = flag_prefix_counts(z, D);
    std::vector<std::vector<Ref>> dg(n, std::vector<Ref>(D));
    for (size_t i = 0; i < n; i++)
        for (size_t q = 0; q < D; q++) {
            if (((size_t)1 << (2 * q)) > i) { dg[i][q] = trivial_block(e_, 0); continue; }   // shift <= i < 4^q
            dg[i][q] = pbs(lin(e_, {{1, &shifts[i][q]}, {4, &z[i]}}), LUT_SEL_F);               // digit unless NUL
        }
    FStr cur = s;
    for (int k = 0; k < K; k++) {
        const size_t d = (size_t)1 << k, q = (size_t)k / 2;
        const bool hi = k & 1;
        // the stage's move flag: bit k of the shift, from its digit; statically 0 where the shift cannot reach 2^k
        std::vector<Ref> mv(n);
        std::vector<bool> moves(n);
        for (size_t p = 0; p < n; p++) {
            if (d > p || (e_->is_triv(dg[p][q].id()) && ((e_->triv_val(dg[p][q].id()) >> (hi ? 1 : 0)) & 1) == 0))
                mv[p] = trivial_block(e_, 0);
            else mv[p] = pbs(dg[p][q], hi ? LUT_BIT1_UNLESS : LUT_BIT0_UNLESS);
            moves[p] = !(e_->is_triv(mv[p].id()) && e_->triv_val(mv[p].id()) == 0);
        }
        // digits still needed after this stage: those holding a bit above k that exists (bits 0 .. K-1)
        size_t q0 = hi ? q + 1 : q;
        if ((size_t)k + 1 >= (size_t)K) q0 = D;              // last stage: nothing travels on
        // the moving part of every block and digit
        FStr md(n);
        std::vector<std::vector<Ref>> mdg(n, std::vector<Ref>(D));
        for (size_t p = 0; p < n; p++) {
            if (!moves[p]) continue;
            for (int blk = 0; blk < 4; blk++) md[p].b[blk] = pbs(lin(e_, {{4, &mv[p]}, {1, &cur[p].b[blk]}}), LUT_SEL_T);
            for (size_t jq = q0; jq < D; jq++) mdg[p][jq] = pbs(lin(e_, {{4, &mv[p]}, {1, &dg[p][jq]}}), LUT_SEL_T);
        }
        FStr nxt(n);
        std::vector<std::vector<Ref>> nd(n, std::vector<Ref>(D));
        for (size_t p = 0; p < n; p++) {
            const bool in = p + d < n && moves[p + d];
            auto combine = [&](const Ref &here, const Ref *out, const Ref *inc) {
                Term tt[3];
                size_t m = 0;
                tt[m++] = {1, here.id()};
                if (out) tt[m++] = {-1, out->id()};
                if (inc) tt[m++] = {1, inc->id()};
                return m == 1 ? here : Ref(e_, e_->lin(tt, m, 0));
            };
            for (int blk = 0; blk < 4; blk++)
                nxt[p].b[blk] = combine(cur[p].b[blk], moves[p] ? &md[p].b[blk] : nullptr, in ? &md[p + d].b[blk] : nullptr);
            for (size_t jq = 0; jq < D; jq++) {
                if (jq < q0) { nd[p][jq] = trivial_block(e_, 0); continue; }
                nd[p][jq] = combine(dg[p][jq], moves[p] ? &mdg[p][jq] : nullptr, in ? &mdg[p + d][jq] : nullptr);
            }
        }
        cur.swap(nxt);
        dg.swap(nd);
    }
    for (size_t p = 0; p < n; p++)                           // hand fresh ciphertexts to whatever comes next
        for (int blk = 0; blk < 4; blk++)
            if (e_->sum_c2(cur[p].b[blk].id()) > 1) cur[p].b[blk] = pbs(cur[p].b[blk], LUT_MSG);
    return cur;
}

FChar Strings::f_eq(const FStr &a, const FStr &b) {
    // (both zero) or equal == equal, so the per-position test of mod.rs:1137-1146 is a plain equality
    std::vector<Ref> f;
    const size_t common = std::min(a.size(), b.size());
    for (size_t i = 0; i < common; i++)
        for (Ref &x : block_eq_flags(a[i], b[i])) f.push_back(x);
    // len(a) == len(b) (mod.rs:1133-1135,1148; len = number of non-zero characters): once every common position holds
    // equal characters the two counts differ exactly by the non-zero characters of the longer buffer's tail, so the
    // condition is "that tail is all zero" -- one digit-sum test per extra character instead of two 8-bit popcounts with
    // their carry chains (eq_ignore_case on 4096 characters: 19 levels / 68 541 bootstraps before)
    const FStr &longer = a.size() > b.size() ? a : b;
    for (size_t i = common; i < longer.size(); i++) f.push_back(char_zero_test(longer[i], true));
    return ch_flag(e_, and_tree(f));
}

// 'A'..'Z' = 0x41..0x5A (high nibble 4: low in 1..15; high nibble 5: low in 0..10); 'a'..'z' = +0x20
Ref Strings::is_upper_flag(const FChar &c, bool lower) {
    Ref lo = lin(e_, {{1, &c.b[0]}, {4, &c.b[1]}});
    Ref hi = lin(e_, {{1, &c.b[2]}, {4, &c.b[3]}});
    Ref row = pbs(hi, lower ? LUT_HI_ROW67 : LUT_HI_ROW45);
    Ref cls = pbs(lo, LUT_EQIC_LO);                          // (low >= 1) + 2 (low <= 10)
    return pbs(lin(e_, {{1, &row}, {4, &cls}}), LUT_CLS_PICK);
}

FStr Strings::f_case(const FStr &s, bool to_lower) {
    FStr r;
    for (const FChar &c : s) {
        Ref f = is_upper_flag(c, /*lower=*/!to_lower);
        FChar o = c;
        o.b[2] = lin(e_, {{1, &c.b[2]}, {to_lower ? 2 : -2, &f}});
        r.push_back(o);
    }
    return r;
}

}  // namespace fhs
