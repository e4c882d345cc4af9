// String layer, part 5 of 7: the fused replace and the split family.
#include "strings.h"

#include <algorithm>
#include <cstring>
#include <set>

#include "strings_internal.h"

namespace fhs {

// ---------------------------------------------------------------------------------------------
// split family (src/server_key/split.rs), same loops as the reference; in fused mode the char-level
// helpers work on single-block flags and the buffers are compacted instead of bubble-sorted
// ---------------------------------------------------------------------------------------------
FChar Strings::s_eq(const FChar &a, const FChar &b) {
    return fused() ? ch_flag(e_, and_tree(block_eq_flags(a, b))) : ch_eq(a, b);
}
FChar Strings::s_ite(const FChar &flag, const FChar &tv, const FChar &fv) {
    return fused() ? ite_flag(flag.b[0], tv, fv) : ch_ite(flag, tv, fv);
}
FChar Strings::s_not(const FChar &flag) {
    if (!fused()) return ch_flip(flag);
    return ch_flag(e_, flag_not(flag.b[0]));
}

FChar Strings::split_match(bool reverse, size_t i, const FStr &s, const FStr &pat, FStr &mask) {
    const FChar zero = t(0), one = t(1);
    FChar found = one;
    if (reverse) {                                           // rsplit_pattern_matching, split.rs:10-67
        if (pat.empty()) {
            FChar cur_pad = s_eq(s[i], zero);
            if (i >= 1) {
                FChar prev_nonpad = s_not(s_eq(s[i - 1], zero));
                found = s_ite(ch_bitand(prev_nonpad, cur_pad), one, zero);
                found = ch_bitor(found, s_ite(cur_pad, zero, one));
            } else found = s_ite(cur_pad, zero, one);
        } else if (pat.size() > s.size() || i + pat.size() >= s.size()) {
            found = zero;
        } else {
            for (size_t j = 0; j < pat.size(); j++) {
                found = ch_bitand(found, s_eq(s[i + j], pat[j]));
                found = ch_bitand(found, mask[i + j]);
            }
        }
    } else {                                                 // split_pattern_matching, split.rs:69-108
        if (pat.size() > s.size() || i + 1 < pat.size()) {
            found = zero;
        } else {
            for (size_t j = 0; j < pat.size(); j++) {
                const size_t k = i + 1 - pat.size() + j;
                found = ch_bitand(found, s_eq(s[k], pat[j]));
                found = ch_bitand(found, mask[k]);
            }
        }
    }
    for (size_t j = 0; j < pat.size(); j++)                  // no overlapping re-match
        if (i + j < s.size()) mask[i + j] = ch_bitand(mask[i + j], s_ite(found, zero, one));
    return found;
}

std::vector<FStr> Strings::xsplit(const FStr &s_in, const FStr &pat, bool inclusive, bool terminator,
                                  const FChar *n, bool reverse, FChar *found_out) {   // _rsplit :307-393, _split :883-988
    const FChar zero = t(0), one = t(1);
    FStr s = s_in;
    s.push_back(zero);
    const size_t size = s.size();
    std::vector<FStr> result(size, FStr(size, zero));
    if (fused() && f_split_distribute(s, pat, n, reverse, result, found_out)) {
        split_cleanup(result, pat, inclusive, terminator, n);
        return result;
    }
    FChar cur_buf = zero, stop_inc = zero, global_found = zero, allow = zero;
    FStr mask(size, one);
    if (n) allow = ch_ne(*n, zero);
    if (!reverse && pat.empty() && n) {                      // split.rs:925-937
        FChar enc_len = len(s)[0];
        FChar skip = ch_bitand(ch_gt(*n, one), ch_le(*n, enc_len));
        cur_buf = s_ite(skip, t(1), cur_buf);
    }
    for (size_t step = 0; step < size; step++) {
        const size_t i = reverse ? size - 1 - step : step;
        for (size_t j = 0; j < size; j++) {                  // copy_logic, split.rs:110-134
            FChar flag = s_eq(t((uint8_t)j), cur_buf);
            if (n) flag = ch_bitand(flag, allow);
            result[j][i] = s_ite(flag, s[i], result[j][i]);
        }
        FChar f = split_match(reverse, i, s, pat, mask);
        global_found = ch_bitor(global_found, f);
        if (!n) {                                            // handle_n_case, split.rs:136-173
            cur_buf = s_ite(f, ch_add(cur_buf, one), cur_buf);
        } else {
            stop_inc = ch_bitor(stop_inc, s_eq(cur_buf, ch_sub(*n, one)));
            cur_buf = s_ite(ch_bitand(f, s_not(stop_inc)), ch_add(cur_buf, one), cur_buf);
        }
    }
    split_cleanup(result, pat, inclusive, terminator, n);
    *found_out = global_found;
    return result;
}

// Runs `op(row, a, b)` on the SUPPORT of a buffer only: leading and trailing characters that are trivially (provably)
// NUL cannot take part in a match of a NUL-free pattern and end up behind the payload after the bubble anyway, so the
// O(L log L) cleanup works on the L positions a buffer can actually receive instead of the whole row.
FStr Strings::on_support(const FStr &row, FStr (Strings::*op)(const FStr &, const FStr &, const FStr &), const FStr &a,
                         const FStr &b) {
    auto triv0 = [&](const FChar &c) {
        for (int k = 0; k < 4; k++)
            if (!e_->is_triv(c.b[k].id()) || e_->triv_val(c.b[k].id()) != 0) return false;
        return true;
    };
    size_t lo = 0, hi = row.size();
    while (lo < hi && triv0(row[lo])) lo++;
    while (hi > lo && triv0(row[hi - 1])) hi--;
    FStr out(row.size(), t(0));
    if (lo == hi) return out;
    FStr sub(row.begin() + lo, row.begin() + hi);
    FStr r = (this->*op)(sub, a, b);
    for (size_t k = 0; k < std::min(r.size(), out.size()); k++) out[k] = r[k];
    return out;
}

// clear_pattern_from_result, split.rs:175-305
void Strings::split_cleanup(std::vector<FStr> &result, const FStr &pat, bool inclusive, bool terminator, const FChar *n) {
    const FChar zero = t(0), one = t(1);
    const size_t size = result.size();
    FStr to(pat.size(), zero);
    // fused mode: the same operations on each buffer's support (see on_support); as written: on the whole row
    auto do_replace = [&](const FStr &row) {
        return fused() ? on_support(row, &Strings::replace, pat, to) : replace(row, pat, to);
    };
    auto bubble3 = [](Strings *S, const FStr &r) { return S->bubble_zeroes_right(r); };
    (void)bubble3;
    auto do_bubble = [&](const FStr &row) {
        if (!fused()) return bubble_zeroes_right(row);
        struct H { static FStr f(Strings *S, const FStr &r) { return S->bubble_zeroes_right(r); } };
        // support trick without the member-pointer signature: trim by hand
        size_t lo = 0, hi = row.size();
        auto triv0 = [&](const FChar &c) {
            for (int k = 0; k < 4; k++)
                if (!e_->is_triv(c.b[k].id()) || e_->triv_val(c.b[k].id()) != 0) return false;
            return true;
        };
        while (lo < hi && triv0(row[lo])) lo++;
        while (hi > lo && triv0(row[hi - 1])) hi--;
        FStr out(row.size(), zero);
        if (lo == hi) return out;
        FStr r = H::f(this, FStr(row.begin() + lo, row.begin() + hi));
        for (size_t k = 0; k < r.size(); k++) out[k] = r[k];
        return out;
    };
    if (n) {
        FChar stop = zero;
        for (size_t i = 0; i < size; i++) {
            stop = ch_bitor(stop, s_eq(*n, ch_add(t((uint8_t)i), one)));
            FStr cur = do_bubble(result[i]);
            FStr rep = do_replace(cur);
            for (size_t j = 0; j < size; j++) result[i][j] = s_ite(stop, cur[j], rep[j]);
        }
    } else {
        for (size_t i = 0; i < size; i++)
            result[i] = inclusive ? do_bubble(result[i]) : do_replace(result[i]);
        if (terminator) {                                    // split.rs:266-302
            FChar nonzero_found = zero;
            for (size_t i = size; i-- > 0;) {
                FChar is_zero = one;
                for (size_t j = 0; j < size; j++) is_zero = ch_bitand(is_zero, s_eq(result[i][j], zero));
                FStr head(result[i].begin(), result[i].begin() + size);
                FChar starts = starts_with(head, pat);
                FChar del = ch_bitand(ch_bitand(starts, is_zero), s_not(nonzero_found));
                for (size_t j = 0; j < size; j++) result[i][j] = s_ite(del, zero, result[i][j]);
                nonzero_found = ch_bitor(nonzero_found, s_not(is_zero));
            }
        }
    }
}

// Fused distribution phase of the split family (split.rs:110-173, :307-393, :883-988 re-associated).
//
// The reference walks the string once; at step t it copies the current character into buffer `cur_buf` (an n x n grid
// of if_then_else on an encrypted u8 index) and then bumps `cur_buf` if a pattern occurrence ends (starts, for the
// reverse family) there and is not masked.  Here:
//   1. window flags for every step at once;
//   2. the mask as a countdown state machine: an accepted occurrence masks positions i .. i+m-1, which blocks the
//      next 2m-2 steps of the forward scan (m-1 of the reverse scan); 2 PBS per step, like the greedy replace;
//   3. cur_buf[t] = number of accepted occurrences before step t = an exclusive prefix count (log depth), as a
//      multi-digit base-4 number, so buffer indices are not limited to a u8; with a limit n (splitn / rsplitn /
//      rsplit_once) the counter stops at n - 1: cur_buf = min(count, n - 1);
//   4. membership of character t in buffer j = AND over the digits of [digit_d(cur_buf) == digit_d(j)] (one shared
//      LUT per digit value and step, one AND per (step, buffer)), only for the buffers step t can reach
//      (j <= ceil(t / (block + 1))), and a 1-PBS-per-block select instead of the 11-PBS equality + if_then_else.
// Returns false (nothing done) for the cases left to the loop above: empty pattern, or a pattern so long that the
// countdown does not fit the LUT (m > 4 forward, m > 8 reverse).
bool Strings::f_split_distribute(const FStr &s, const FStr &pat, const FChar *n, bool reverse, std::vector<FStr> &result,
                                 FChar *found_out) {
    const size_t size = s.size(), m = pat.size();
    if (m == 0) return false;
    const size_t block = reverse ? m - 1 : 2 * m - 2;        // steps blocked after an accepted occurrence
    if (block > 7) return false;
    const FChar zero = t(0), one = t(1);
    auto pos = [&](size_t step) { return reverse ? size - 1 - step : step; };

    // 1. window flags in scan order
    std::vector<Ref> w(size);
    for (size_t step = 0; step < size; step++) {
        const size_t i = pos(step);
        if (m > size) { w[step] = trivial_block(e_, 0); continue; }
        if (reverse) w[step] = i + m < size ? window_match(s, i, pat) : trivial_block(e_, 0);          // :47-49
        else w[step] = i + 1 >= m ? window_match(s, i + 1 - m, pat) : trivial_block(e_, 0);            // :85-87
    }
    // 2. accepted occurrences
    std::vector<Ref> f(size);
    if (block == 0) f = w;
    else {
        Ref state = trivial_block(e_, 0);
        for (size_t step = 0; step < size; step++) {
            Ref v = lin(e_, {{2, &state}, {1, &w[step]}});
            f[step] = pbs(v, LUT_GREEDY_SEL);
            state = pbs(v, LUT_GREEDY_NEXT0 + (int)block);
        }
    }
    *found_out = ch_flag(e_, or_tree(f));

    // 3. buffer index of every step
    const size_t max_count = (size + block) / (block + 1);   // occurrences are at least block + 1 steps apart
    size_t D = 1;
    while (((size_t)1 << (2 * D)) <= max_count) D++;
    if (n) D = std::max<size_t>(D, 4);
    std::vector<Num> cur = flag_prefix_counts(f, D);
    Ref allow;
    if (n) {
        allow = blk_nonzero_flag(*n);                        // n == 0: nothing is ever copied (:124-127)
        FChar n1 = ch_sub(*n, one);                          // the counter stops at n - 1 (u8 arithmetic, :153-157)
        for (size_t step = 0; step < size; step++) {
            FChar low;
            for (int d = 0; d < 4; d++) low.b[d] = cur[step][d];
            Ref lt = blk_cmp_flag(low, n1, LUT_CMP_LT);      // count < n - 1 on the low 4 digits
            if (D > 4) {
                Term tt[16];
                size_t k = 0;
                for (size_t d = 4; d < D; d++) tt[k++] = {1, cur[step][d].id()};
                Ref hi0 = pbs(Ref(e_, e_->lin(tt, k, 0)), LUT_IS0);
                lt = pbs(lin(e_, {{1, &lt}, {1, &hi0}}), LUT_IS2);
            }
            Num clamped(D);
            for (size_t d = 0; d < D; d++) {
                Ref a = pbs(lin(e_, {{4, &lt}, {1, &cur[step][d]}}), LUT_SEL_T);
                if (d < 4) {
                    Ref b = pbs(lin(e_, {{4, &lt}, {1, &n1.b[d]}}), LUT_SEL_F);
                    clamped[d] = lin(e_, {{1, &a}, {1, &b}});
                } else clamped[d] = a;
            }
            cur[step] = clamped;
        }
    }

    // 4. membership and copy
    for (size_t step = 0; step < size; step++) {
        const size_t i = pos(step);
        size_t jmax = std::min(size - 1, (step + block) / (block + 1));
        std::vector<Ref> q(D * 4);                           // q[4 d + v] = [digit d of cur_buf == v], made on demand
        auto digit_flag = [&](size_t d, int v) -> Ref & {
            Ref &r = q[4 * d + v];
            if (!r) r = pbs(cur[step][d], lut_is_k(v));
            return r;
        };
        for (size_t j = 0; j <= jmax; j++) {
            if ((j >> (2 * D)) != 0) break;                  // not representable: unreachable by construction
            std::vector<Ref> fl;
            for (size_t d = 0; d < D; d++) fl.push_back(digit_flag(d, (int)((j >> (2 * d)) & 3)));
            if (n) fl.push_back(allow);
            Ref mem = and_tree(fl);
            if (e_->is_triv(mem.id()) && e_->triv_val(mem.id()) == 0) continue;
            for (int b = 0; b < 4; b++) result[j][i].b[b] = pbs(lin(e_, {{4, &mem}, {1, &s[i].b[b]}}), LUT_SEL_T);
        }
    }
    return true;
}

std::vector<FStr> Strings::split_ws(const FStr &s, FChar *found_out) {   // split.rs:1377-1447
    const FChar zero = t(0), one = t(1);
    const size_t size = s.size();
    FChar cur_buf = zero, prev_ws = t(1), global_found = zero;
    std::vector<FStr> result(size, FStr(size, zero));
    auto is_ws = [&](const FChar &c) {
        if (!fused()) return ch_is_whitespace(c);
        // significant = neither NUL nor whitespace; whitespace = !significant & nonzero
        Ref sig = char_significant(c), nz = char_zero_test(c, false);
        return ch_flag(e_, lin(e_, {{1, &nz}, {-1, &sig}}));
    };
    for (size_t i = 0; i < size; i++) {
        FChar f = is_ws(s[i]);
        global_found = ch_bitor(global_found, f);
        FChar inc = ch_bitand(f, s_not(prev_ws));
        cur_buf = s_ite(inc, ch_add(cur_buf, one), cur_buf);
        FChar not_ws = s_not(f);
        for (size_t j = 0; j < size; j++) {
            FChar flag = ch_bitand(s_eq(t((uint8_t)j), cur_buf), not_ws);
            result[j][i] = s_ite(flag, s[i], result[j][i]);
        }
        prev_ws = f;
    }
    // (:1428-1436 re-tests every buffer char for whitespace: only non-whitespace was ever copied)
    for (size_t j = 0; j < size; j++) result[j] = bubble_zeroes_right(result[j]);
    *found_out = global_found;
    return result;
}

std::vector<FStr> Strings::split_family(int kind, const FStr &s, const FStr &pat, const FChar *n, FChar *found) {
    const FChar two = t(2);
    switch (kind) {
        case SPLIT: return xsplit(s, pat, false, false, nullptr, false, found);             // split.rs:989
        case SPLIT_INCLUSIVE: return xsplit(s, pat, true, false, nullptr, false, found);    // :1020
        case SPLIT_TERMINATOR: return xsplit(s, pat, false, true, nullptr, false, found);   // :1051
        case SPLITN: return xsplit(s, pat, false, false, n, false, found);                  // :1448
        case RSPLIT: return xsplit(s, pat, false, false, nullptr, true, found);             // :394
        case RSPLIT_TERMINATOR: return xsplit(s, pat, false, true, nullptr, true, found);   // :504
        case RSPLITN: return xsplit(s, pat, false, false, n, true, found);                  // :421
        case RSPLIT_ONCE: return xsplit(s, pat, false, false, &two, true, found);           // :462
        default: return split_ws(s, found);                                                 // :1377
    }
}

// replace with |from| < |to| (handle_shorter_from, mod.rs:885-980) re-associated.  The reference scans
// left to right, splices `to` in place and masks the inserted text, i.e. it replaces the greedy
// leftmost NON-overlapping matches.  Here: match flags on the original string; a countdown state
// machine (1 block, 2 PBS per position) picks the greedy matches; every position then emits a slot of
// |to| characters (`to` at a selected start, nothing inside a match, itself otherwise) and the slots
// are compacted.  Same plaintext as the reference; the buffer is (n+1)*|to| chars instead of
// |to|*(n+1) + (n+1).
FStr Strings::f_replace_expand(const FStr &s_in, const FStr &from, const FStr &to) {
    const FChar zero = t(0);
    FStr s = s_in;
    s.push_back(zero);                                       // :898
    const size_t n = s.size(), m = from.size(), L = to.size();
    std::vector<Ref> sel(n), covered(n), keep_flag(n);
    Ref state = trivial_block(e_, 0);                        // positions still blocked by the last match
    // 1 - sel - covered is a sum of m outputs and enters the select below with weight 4: 16 m + 1 > 64 from m = 4 on.
    // The same flag is [countdown == 0 and no match here] = [v == 0], one more look-up on the state machine's own input
    // (same dependency level, sum c^2 = 5), used from the pattern length on where the linear form leaves the budget.
    const bool keep_by_lut = 16 * (int64_t)m + 1 > FHS_NOISE_BUDGET_SUM_C2;
    for (size_t i = 0; i < n; i++) {
        Ref f = i + m <= n ? window_match(s, i, from) : trivial_block(e_, 0);
        Ref v = lin(e_, {{2, &state}, {1, &f}});
        sel[i] = pbs(v, LUT_GREEDY_SEL);
        if (keep_by_lut) keep_flag[i] = pbs(v, LUT_IS0);
        state = pbs(v, LUT_GREEDY_NEXT0 + (int)(m - 1));     // selected ? m - 1 : max(countdown - 1, 0)
    }
    for (size_t i = 0; i < n; i++) {
        Term tt[8];
        size_t k = 0;
        for (size_t d = 1; d < m && d <= i; d++) tt[k++] = {1, sel[i - d].id()};
        covered[i] = Ref(e_, e_->lin(tt, k, 0));             // inside a selected match (not its start)
    }
    Ref one = trivial_block(e_, 1);
    FStr slots;
    slots.reserve(n * L);
    for (size_t i = 0; i < n; i++) {
        Ref keep = keep_by_lut ? keep_flag[i] : lin(e_, {{1, &one}, {-1, &sel[i]}, {-1, &covered[i]}});
        for (size_t j = 0; j < L; j++) {
            FChar c;
            for (int b = 0; b < 4; b++) {
                Ref a = pbs(lin(e_, {{4, &sel[i]}, {1, &to[j].b[b]}}), LUT_SEL_T);
                if (j == 0) {
                    Ref o = pbs(lin(e_, {{4, &keep}, {1, &s[i].b[b]}}), LUT_SEL_T);
                    c.b[b] = lin(e_, {{1, &a}, {1, &o}});
                } else c.b[b] = a;
            }
            slots.push_back(c);
        }
    }
    return f_compact(slots);
}

}  // namespace fhs
