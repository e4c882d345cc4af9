// String layer, part 1 of 7: the as-written mirror of the reference's methods (strings.h lists the parts' sections).
#include "strings.h"

#include <algorithm>
#include <cstring>
#include <set>

#include "strings_internal.h"

namespace fhs {

FStr Strings::clear(const char *s, size_t n) const {
    FStr r;
    for (size_t i = 0; i < n; i++) r.push_back(t((uint8_t)s[i]));
    return r;
}

// ---------------------------------------------------------------------------------------------
// as written (same op sequence as the reference; cf. oracle/strings.py)
// ---------------------------------------------------------------------------------------------
FStr Strings::bubble_zeroes_right(const FStr &in) {          // utils.rs:28-46
    if (fused()) return f_compact(in);
    FStr s = in;
    const FChar zero = t(0);
    for (size_t pass = 0; pass < s.size(); pass++)
        for (size_t i = 0; i + 1 < s.size(); i++) {
            FChar swap = ch_eq(s[i], zero);
            FChar a = ch_ite(swap, s[i + 1], s[i]);
            FChar b = ch_ite(swap, zero, s[i + 1]);
            s[i] = a;
            s[i + 1] = b;
        }
    return s;
}

FStr Strings::to_upper(const FStr &s) {                      // mod.rs:65-84
    if (fused()) return f_case(s, false);
    const FChar zero = t(0), cst = t(32);
    FStr r;
    for (const FChar &b : s) r.push_back(ch_sub(b, ch_ite(ch_flip(ch_is_lowercase(b)), zero, cst)));
    return r;
}
FStr Strings::to_lower(const FStr &s) {                      // mod.rs:110-128
    if (fused()) return f_case(s, true);
    const FChar zero = t(0), cst = t(32);
    FStr r;
    for (const FChar &b : s) r.push_back(ch_add(b, ch_ite(ch_flip(ch_is_uppercase(b)), zero, cst)));
    return r;
}

FChar Strings::contains(const FStr &s, const FStr &needle) { // mod.rs:151-182
    if (s.empty() && needle.empty()) return t(1);
    if (needle.size() > s.size()) return t(0);
    if (fused()) return f_contains(s, needle);
    FChar result = t(0);
    const FChar one = t(1);
    for (size_t i = 0; i + needle.size() <= s.size(); i++) {
        FChar cur = one;
        for (size_t j = 0; j < needle.size(); j++) cur = ch_bitand(cur, ch_eq(s[i + j], needle[j]));
        result = ch_bitor(result, cur);
    }
    return result;
}

FChar Strings::ends_with(const FStr &s, const FStr &needle) {   // mod.rs:241-288
    if (s.empty() && needle.empty()) return t(1);
    if (needle.size() > s.size()) return t(0);
    if (fused()) return f_ends_with(s, needle, nullptr);
    FChar result = t(0);
    const FChar one = t(1), zero = t(0);
    for (size_t i = 0; i + needle.size() <= s.size(); i++) {
        FChar cur = one, nonzero = one;
        for (size_t j = 0; j < needle.size(); j++) {
            cur = ch_bitand(cur, ch_eq(s[i + j], needle[j]));
            nonzero = ch_bitand(nonzero, ch_ne(s[i + j], zero));
        }
        result = ch_ite(nonzero, cur, result);
    }
    return result;
}

FChar Strings::starts_with(const FStr &s, const FStr &pat) { // mod.rs:344-371
    if (pat.size() > s.size()) return t(0);
    if (s.empty() && pat.empty()) return t(1);
    if (fused()) {
        if (pat.empty()) return t(1);
        return ch_flag(e_, window_match(s, 0, pat));
    }
    FChar result = t(1);
    for (size_t i = 0; i < std::min(pat.size(), s.size()); i++) result = ch_bitand(result, ch_eq(s[i], pat[i]));
    return result;
}

FChar Strings::is_empty(const FStr &s) {                     // mod.rs:431-451
    if (s.empty()) return t(1);
    const FChar zero = t(0);
    if (fused()) {
        std::vector<Ref> f;
        for (const FChar &c : s) f.push_back(char_zero_test(c, true));
        return ch_flag(e_, and_tree(f));
    }
    FChar result = t(1);
    for (const FChar &c : s) result = ch_bitand(result, ch_eq(c, zero));
    return result;
}

FStr Strings::repeat_clear(const FStr &s, size_t n) {        // mod.rs:517-538
    if (n == 0) return {};
    FStr r;
    for (size_t k = 0; k < n; k++) r.insert(r.end(), s.begin(), s.end());
    return bubble_zeroes_right(r);
}

FStr Strings::repeat(const FStr &s, const FChar &n) {        // mod.rs:567-591
    const FChar zero = t(0);
    FStr r(FHS_MAX_REPETITIONS * s.size(), zero);
    for (size_t i = 0; i < FHS_MAX_REPETITIONS; i++) {
        FChar flag = ch_lt(t((uint8_t)i), n);
        for (size_t j = 0; j < s.size(); j++) r[i * s.size() + j] = ch_ite(flag, s[j], zero);
    }
    return bubble_zeroes_right(r);
}

FStr Strings::replace(const FStr &s, const FStr &from, const FStr &to) {   // mod.rs:624-653
    const FChar n = t(0);
    if (from.size() >= to.size()) return longer_from(s, from, to, n, false);
    return shorter_from(s, from, to, n, false);
}
FStr Strings::replacen(const FStr &s, const FStr &from, const FStr &to, const FChar &n) {   // mod.rs:1729-1757
    if (from.size() >= to.size()) return longer_from(s, from, to, n, true);
    return shorter_from(s, from, to, n, true);
}

FStr Strings::longer_from(const FStr &s, const FStr &from, FStr to, const FChar &n, bool use_counter) {   // mod.rs:828-882
    const FChar zero = t(0), one = t(1);
    FStr data = s;
    data.push_back(zero);                                   // :841
    while (to.size() < from.size()) to.push_back(zero);     // :847-849
    FChar counter = t(0);
    FStr result = data;
    if (fused() && !use_counter && !from.empty() && from.size() <= 10 && from.size() <= result.size()) {
        // The loop below writes `to` over every matching window in ascending order, flags taken on the ORIGINAL data: the
        // LAST matching window that covers a position wins.  Re-associated per position p: sel_k = window p-k matches and
        // none of p-k+1 .. p does (one bootstrap each on 5 * match[p-k] + the later flags: equals 5 exactly then), none =
        // no window covers p; result[p] = none ? data[p] : to[the k that is set] -- (m + 1) selects per block instead of
        // 2 m, two levels deep instead of m chained ones.
        const size_t m = from.size(), end = adjust_end_of_pattern(result.size() - from.size());
        std::vector<Ref> match(end);
        for (size_t i = 0; i < end; i++) match[i] = window_match(data, i, from);
        for (size_t p = 0; p < result.size(); p++) {
            std::vector<Ref> later;                          // match flags of windows p-j, j < k, that exist
            std::vector<std::pair<size_t, Ref>> sel;         // (k, flag)
            for (size_t k = 0; k < m && k <= p; k++) {
                const size_t i = p - k;
                if (i >= end) continue;
                if (later.empty()) sel.push_back({k, match[i]});
                else {
                    Term tt[12];
                    size_t c = 0;
                    tt[c++] = {5, match[i].id()};
                    for (const Ref &l : later) tt[c++] = {1, l.id()};
                    sel.push_back({k, pbs(Ref(e_, e_->lin(tt, c, 0)), lut_is_k(5))});
                }
                later.push_back(match[i]);
            }
            if (sel.empty()) continue;                       // no window reaches this position
            Ref none = pbs(sum_refs(e_, later.data(), later.size()), lut_is_k(0));
            for (int b = 0; b < 4; b++) {
                Term tt[12];
                size_t c = 0;
                Ref keepv = pbs(lin(e_, {{4, &none}, {1, &data[p].b[b]}}), LUT_SEL_T);
                std::vector<Ref> parts{keepv};
                for (auto &kv : sel) parts.push_back(pbs(lin(e_, {{4, &kv.second}, {1, &to[kv.first].b[b]}}), LUT_SEL_T));
                for (const Ref &x : parts) tt[c++] = {1, x.id()};
                result[p].b[b] = Ref(e_, e_->lin(tt, c, 0));
            }
        }
        return bubble_zeroes_right(result);                 // :881
    }
    if (from.size() <= result.size()) {
        const size_t end = adjust_end_of_pattern(result.size() - from.size());
        for (size_t i = 0; i < end; i++) {
            FChar flag = one;
            if (fused() && !from.empty()) flag = ch_flag(e_, window_match(data, i, from));
            else for (size_t j = 0; j < from.size(); j++) flag = ch_bitand(flag, ch_eq(from[j], data[i + j]));
            if (use_counter) {                              // :868-872
                counter = ch_add(counter, flag);
                flag = ch_bitand(flag, ch_ge(n, counter));
            }
            for (size_t k = 0; k < to.size(); k++)
                result[i + k] = fused() ? ite_flag(flag.b[0], to[k], result[i + k]) : ch_ite(flag, to[k], result[i + k]);
        }
    }
    return bubble_zeroes_right(result);                     // :881
}

FStr Strings::shorter_from(const FStr &s, const FStr &from, const FStr &to, const FChar &n, bool use_counter) {   // mod.rs:885-980
    if (fused() && !use_counter && !from.empty() && from.size() <= 8) return f_replace_expand(s, from, to);
    const FChar zero = t(0), one = t(1);
    FStr data = s;
    data.push_back(zero);
    const size_t size_diff = to.size() - from.size();
    FChar counter = t(0);
    size_t max_len = data.empty() ? to.size() : to.size() * data.size() + data.size();
    if (from.empty()) max_len = (data.size() + (data.size() + 1) * to.size()) + 1;
    FStr result = data;
    result.resize(max_len, zero);
    FStr copy_buffer(max_len, zero);
    FStr ignore_mask(max_len, one);
    for (size_t i = 0; i + to.size() < result.size(); i++) {
        FChar flag = one;
        for (size_t j = 0; j < from.size(); j++) {
            flag = ch_bitand(flag, ch_eq(from[j], result[i + j]));
            flag = ch_bitand(flag, ignore_mask[i + j]);
        }
        if (from.empty()) flag = (i % (to.size() + 1) == 0) ? one : zero;
        if (use_counter) {
            counter = ch_add(counter, flag);
            flag = ch_bitand(flag, ch_ge(n, counter));
        }
        for (size_t k = 0; k < max_len; k++) copy_buffer[k] = ch_ite(flag, result[k], zero);
        for (size_t k = 0; k < to.size(); k++) {
            result[i + k] = ch_ite(flag, to[k], result[i + k]);
            ignore_mask[i + k] = ch_bitand(ignore_mask[i + k], ch_ite(flag, zero, one));
        }
        for (size_t k = i + to.size(); k < max_len; k++)
            result[k] = ch_ite(flag, copy_buffer[k - size_diff], result[k]);
    }
    return result;
}

FChar Strings::eq(const FStr &a, const FStr &b) {            // mod.rs:1122-1149
    if (fused()) return f_eq(a, b);
    const FChar zero = t(0), one = t(1);
    FChar is_eq = one;
    FChar len_ne = ch_ne(len(a)[0], len(b)[0]);
    for (size_t i = 0; i < std::min(a.size(), b.size()); i++) {
        FChar same = ch_eq(a[i], b[i]);
        FChar both0 = ch_bitand(ch_eq(a[i], zero), ch_eq(b[i], zero));
        is_eq = ch_bitand(is_eq, ch_bitor(both0, same));
    }
    return ch_ite(len_ne, zero, is_eq);
}
FChar Strings::ne(const FStr &a, const FStr &b) {            // mod.rs:1178-1186
    FChar r = eq(a, b);
    if (fused()) return ch_flag(e_, flag_not(r.b[0]));      // on the single live block, no PBS
    return ch_flip(r);
}
FChar Strings::eq_ignore_case(const FStr &a, const FStr &b) {   // mod.rs:1221-1231
    if (fused()) return f_eq_ignore_case(a, b);
    return eq(to_lower(a), to_lower(b));
}

FStr Strings::strip_prefix(const FStr &s, const FStr &pat, FChar *found) {   // mod.rs:1261-1307
    const FChar zero = t(0), one = t(1);
    FStr result = s;
    FChar flag = one;
    const size_t end = std::min(pat.size(), result.size());
    if (pat.size() > result.size()) {
        *found = zero;
        return result;
    }
    if (end == 0 && !pat.empty() && s.empty()) flag = zero;
    for (size_t j = 0; j < end; j++) flag = ch_bitand(flag, ch_eq(pat[j], result[j]));
    for (size_t j = 0; j < std::min(pat.size(), result.size()); j++) result[j] = ch_ite(flag, zero, result[j]);
    *found = flag;
    return bubble_zeroes_right(result);
}

FStr Strings::strip_suffix(const FStr &s_in, const FStr &needle, FChar *found) {   // mod.rs:1335-1404
    const FChar one = t(1), zero = t(0), t255 = t(255);
    FStr s = s_in;
    if (needle.size() > s.size()) {
        *found = zero;
        return s;
    }
    const size_t end = s.size() - needle.size();
    if (fused()) {
        // pos == i exactly for the window picked by ends_with (last window without padding, if it matches)
        std::vector<Ref> pick;
        FChar r = f_ends_with(s, needle, &pick);
        *found = r;
        for (size_t k = 0; k < s.size(); k++) {
            std::vector<Ref> cover;   // windows that contain position k; at most one pick is set overall
            for (size_t i = (k + 1 >= needle.size() ? k + 1 - needle.size() : 0); i <= std::min(k, end); i++)
                cover.push_back(pick[i]);
            if (cover.empty()) continue;
            Ref zk = cover.size() <= 15 ? sum_refs(e_, cover.data(), cover.size()) : or_tree(cover);
            s[k] = ite_flag(zk, zero, s[k]);
        }
        return s;
    }
    FChar pos = t(255);
    for (size_t i = 0; i <= end; i++) {
        FChar fnd = one, nonzero = one;
        for (size_t j = 0; j < needle.size(); j++) {
            fnd = ch_bitand(fnd, ch_eq(s[i + j], needle[j]));
            nonzero = ch_bitand(nonzero, ch_ne(s[i + j], zero));
        }
        FChar cur = ch_ite(fnd, t((uint8_t)i), t255);
        pos = ch_ite(nonzero, cur, pos);
    }
    *found = ch_ne(pos, t255);
    for (size_t i = 0; i <= end; i++) {
        FChar mask = ch_eq(t((uint8_t)i), pos);
        for (size_t j = 0; j < needle.size(); j++) s[i + j] = ch_ite(mask, zero, s[i + j]);
    }
    return s;
}

FChar Strings::comparison(const FStr &a_in, const FStr &b_in, int cmp) {   // mod.rs:1470-1541
    if (fused()) return f_comparison(a_in, b_in, cmp);
    const FChar zero = t(0), t255 = t(255);
    FStr a = a_in, b = b_in;
    size_t min_len = std::min(a.size(), b.size());
    FChar seen = zero, became = zero, ret = t(255);
    if (min_len == 0) {                                      // :1490-1494
        a.push_back(zero);
        b.push_back(zero);
        min_len = 1;
    }
    auto op = [&](const FChar &x, const FChar &y) {
        switch (cmp) {
            case 0: return ch_lt(x, y);
            case 1: return ch_le(x, y);
            case 2: return ch_gt(x, y);
            default: return ch_ge(x, y);
        }
    };
    for (size_t i = 0; i < min_len; i++) {
        FChar c = op(a[i], b[i]);
        seen = ch_bitor(seen, ch_ne(a[i], b[i]));
        FChar flag = ch_bitand(seen, ch_flip(became));
        became = ch_bitor(became, flag);
        ret = ch_ite(flag, c, ret);
    }
    FChar sub_eq = ch_eq(ret, t255);
    FChar l1 = len(a)[0], l2 = len(b)[0];
    FChar leq = ch_eq(l1, l2), lgt = ch_gt(l1, l2), llt = ch_lt(l1, l2);
    FChar by_len;
    switch (cmp) {
        case 3: by_len = ch_bitor(leq, lgt); break;
        case 1: by_len = ch_bitor(leq, llt); break;
        case 2: by_len = lgt; break;
        default: by_len = llt; break;
    }
    return ch_ite(sub_eq, by_len, ret);
}

FStr Strings::concatenate(const FStr &a, const FStr &b) {    // mod.rs:1864-1875
    FStr r = a;
    r.insert(r.end(), b.begin(), b.end());
    return bubble_zeroes_right(r);
}

FStr Strings::trim_end(const FStr &s) {                      // trim.rs:36-57
    if (fused()) return f_trim(s, true);
    const FChar zero = t(0);
    FChar stop = zero;
    FStr r(s.size(), zero);
    for (size_t i = s.size(); i-- > 0;) {
        FChar not_ws = ch_flip(ch_is_whitespace(s[i]));
        stop = ch_bitor(stop, ch_bitand(not_ws, ch_ne(s[i], zero)));
        r[i] = ch_ite(stop, s[i], zero);
    }
    return r;
}
FStr Strings::trim_start(const FStr &s) {                    // trim.rs:86-115
    if (fused()) return f_compact(f_trim(s, false));
    const FChar zero = t(0);
    FChar stop = zero;
    FStr r(s.size(), zero);
    for (size_t i = 0; i < s.size(); i++) {
        FChar not_ws = ch_flip(ch_is_whitespace(s[i]));
        stop = ch_bitor(stop, ch_bitand(not_ws, ch_ne(s[i], zero)));
        r[i] = ch_ite(stop, s[i], zero);
    }
    return bubble_zeroes_right(r);
}
FStr Strings::trim(const FStr &s) { return trim_start(trim_end(s)); }   // trim.rs:146-149

}  // namespace fhs
