// String layer, part 3 of 7: positions and counts -- find, rfind, len, flag counts -- and positions as operands.
#include "strings.h"

#include <algorithm>
#include <cstring>
#include <set>

#include "strings_internal.h"

namespace fhs {

// ---------------------------------------------------------------------------------------------
// positions and counts: find, rfind, len and the flag count, each written once for a result of one half (the reference's
// u8: absent = 255, strings below 255 + |pattern| characters) or two (lo, hi: absent = 65535, below 65535 + |pattern|).
// Everything else is the reference's, quirks included (src/main.rs:20, mod.rs:742-744, :1025-1027, :1044).
// ---------------------------------------------------------------------------------------------
bool Strings::limit_reached(size_t n, size_t m, size_t halves) {
    return n >= (size_t)(halves == 1 ? FHS_MAX_FIND_LENGTH : FHS_MAX_FIND_LENGTH_WIDE) + m;
}

Pos Strings::pos_trivial(unsigned v, size_t halves) const {
    Pos p;
    for (size_t h = 0; h < halves; h++) p.push_back(t((uint8_t)(v >> (8 * h))));
    return p;
}

FChar Strings::num_char(const Num &v, size_t first) {
    FChar c;
    for (int k = 0; k < 4; k++) c.b[k] = v[first + k];
    return c;
}
Pos Strings::num_pos(const Num &v) {
    Pos p;
    for (size_t first = 0; first + 4 <= v.size(); first += 4) p.push_back(num_char(v, first));
    return p;
}

// as written: pos = flag ? v : pos, one if_then_else per half
void Strings::pos_set_if(Pos &pos, const FChar &flag, size_t v) {
    for (size_t h = 0; h < pos.size(); h++) pos[h] = ch_ite(flag, t((uint8_t)(v >> (8 * h))), pos[h]);
}

// as written: counter += flag; with two halves the carry is the wrap of the low one
void Strings::pos_add_flag(Pos &counter, const FChar &flag) {
    FChar lo = ch_add(counter[0], flag);
    if (counter.size() > 1) counter[1] = ch_add(counter[1], ch_lt(lo, counter[0]));
    counter[0] = lo;
}

// as written: AND_j eq(pat[j], s[at + j]), chained from the last j down (find) or from the first up (rfind)
FChar Strings::window_eq(const FStr &s, size_t at, const FStr &pat, bool downwards) {
    FChar flag = t(1);
    for (size_t k = 0; k < pat.size(); k++) {
        const size_t j = downwards ? pat.size() - 1 - k : k;
        flag = ch_bitand(flag, ch_eq(pat[j], s[at + j]));
    }
    return flag;
}

Pos Strings::rfind(const FStr &s_in, const FStr &pat, size_t halves) {   // mod.rs:727-790
    const FChar zero = t(0);
    FStr s = s_in;
    s.push_back(zero);                                       // :737
    if (limit_reached(s.size(), pat.size(), halves)) {       // :742-744
        err = {FHS_ERR_LIMIT, LIMIT_MSG};
        return pos_trivial(0, halves);
    }
    if (fused()) return num_pos(f_rfind_digits(s, pat, 4 * halves));
    if (pat.empty()) {                                       // :747-760
        Pos last = pos_trivial(0, halves);
        for (size_t i = 0; i < s.size(); i++) pos_set_if(last, ch_ne(s[i], zero), i + 1);
        return last;
    }
    Pos pos = pos_trivial(absent_value(halves), halves);
    if (pat.size() > s.size()) return pos;
    const size_t end = adjust_end_of_pattern(s.size() - pat.size());
    for (size_t i = 0; i < end; i++) pos_set_if(pos, window_eq(s, i, pat, false), i);
    return pos;
}

Pos Strings::find(const FStr &s, const FStr &pat, size_t halves) {       // mod.rs:1010-1053
    if (s.empty() && pat.empty()) return pos_trivial(0, halves);
    if (limit_reached(s.size(), pat.size(), halves)) {       // :1025-1027
        err = {FHS_ERR_LIMIT, LIMIT_MSG};
        return pos_trivial(0, halves);
    }
    Pos pos = pos_trivial(absent_value(halves), halves);
    if (pat.size() > s.size()) return pos;
    if (fused()) return num_pos(f_find_digits(f_find_window_flags(s, pat), 4 * halves));
    for (size_t i = s.size() - pat.size() + 1; i-- > 0;) pos_set_if(pos, window_eq(s, i, pat, true), i);
    return pos;
}

// len counts the characters that are not NUL (mod.rs:478-493), count_flags the 0/1 flag chars that are set
Pos Strings::count(const FStr &s, bool are_flags, size_t halves) {
    if (s.empty()) return pos_trivial(0, halves);
    if (fused()) {
        std::vector<Ref> f;
        for (const FChar &c : s) f.push_back(are_flags ? c.b[0] : char_zero_test(c, false));
        return num_pos(count_flags(f, 4 * halves));
    }
    const FChar zero = t(0);
    Pos result = pos_trivial(0, halves);
    for (const FChar &c : s) pos_add_flag(result, are_flags ? c : ch_ne(c, zero));
    return result;
}
Pos Strings::len(const FStr &s, size_t halves) { return count(s, false, halves); }
Pos Strings::count_flags(const FStr &flags, size_t halves) { return count(flags, true, halves); }

// find (mod.rs:1010-1053) re-associated: window flags, exclusive prefix OR, and the index of the first flag set from
// the prefix ORs (first_index), 255 / 65535 when absent.
// The match flag of every window of `s` (the first two dependency levels of find: nibble tests, AND per window)
std::vector<Ref> Strings::f_find_window_flags(const FStr &s, const FStr &pat) {
    if (s.size() < pat.size()) return {};
    const size_t W = s.size() - pat.size() + 1;
    std::vector<Ref> f(W);
    for (size_t i = 0; i < W; i++) f[i] = pat.empty() ? trivial_block(e_, 1) : window_match(s, i, pat);
    return f;
}

// ... and the rest of find on ALL window flags in string order: index of the first one set as 4 or 8 digits (at most
// 4^digits flags: the limit on the string's length sees to that), every digit 3 if none.
Strings::Num Strings::f_find_digits(const std::vector<Ref> &f, size_t digits) {
    std::vector<Ref> p = prefix_or(f);
    Ref found = or_tree(f);
    return first_index(p, found, digits);
}

// The sharded find exchanges the flags and runs this part on every rank (fhs_dist_str_find): a u8 position, 255 if none
FChar Strings::f_find_from_flags(const std::vector<Ref> &f) { return num_char(f_find_digits(f, 4)); }

// Index of the first set flag from the exclusive prefix ORs before[j] = OR(f[0 .. j-1]) (before[W] = found): the flags
// g[j] = found - before[j] = [the first match sits at index >= j] form a thermometer, so floor(index / 4^d) = sum_r
// g[r 4^d] and every base-4 digit is LINEAR in the prefix ORs,
//     digit_d = sum_q L_q,   L_q = g[(4q+1) S] + g[(4q+2) S] + g[(4q+3) S] - 3 g[(4q+4) S],   S = 4^d,
// with at most one block q non-zero (`found` cancels inside a block).  The two high digits are used as they are, the
// low ones refresh their blocks first (noise budget); 255 when nothing is set.  ~90 bootstraps in 1-3 levels instead of
// the one-hot route (first = f & !before, weighted sums: ~560 in 6) -- find on 256 characters: 8 levels instead of 11.
// With `digits` = 8 the same formulas give a 16-bit index (S up to 4^7, W <= 65536, absent 3 x 8 = 65535): a digit whose
// S exceeds W has no block and is 3 nf alone, so a short string pays nothing for the four high digits.
Strings::Num Strings::first_index(const std::vector<Ref> &before, const Ref &found, size_t digits) {
    const size_t W = before.size();                          // index in [0, W), W <= 4^digits
    Ref nf = flag_not(found);
    auto g_terms = [&](size_t j, int64_t coef, std::vector<Term> &tt) {       // coef * g[j], j >= 1
        if (j > W) return;                                   // index >= j is impossible
        tt.push_back({coef, found.id()});
        tt.push_back({-coef, j == W ? found.id() : before[j].id()});
    };
    Num r(digits);
    for (size_t d = 0; d < digits; d++) {
        const size_t S = (size_t)1 << (2 * d);
        std::vector<Ref> blocks;                             // L_q, values 0..3, at most one non-zero
        for (size_t q = 0; (4 * q + 1) * S <= W; q++) {
            std::vector<Term> tt;
            for (size_t i = 1; i <= 3; i++) g_terms((4 * q + i) * S, 1, tt);
            g_terms((4 * q + 4) * S, -3, tt);
            blocks.push_back(Ref(e_, e_->lin(tt.data(), tt.size(), 0)));
        }
        // add the blocks up within the noise budget: while the whole sum (+ the `absent` term) would pass it, merge
        // neighbours up to sum c^2 <= 60 and refresh each merged group (one value in 0..3: at most one block is non-zero)
        // (variances are those of the SUMS: blocks of a mostly plaintext string share bootstrap outputs, their
        // coefficients add up inside a sum)
        auto var_of = [&](const std::vector<Ref> &v) {
            return v.empty() ? (int64_t)0 : e_->sum_c2(v.size() == 1 ? v[0].id() : sum_refs(e_, v.data(), v.size()).id());
        };
        bool stalled_before = false;
        for (;;) {
            if (blocks.size() <= 1 || var_of(blocks) + 9 <= 48) break;
            std::vector<Ref> nxt, grp;
            auto close = [&] {
                if (grp.empty()) return;
                nxt.push_back(pbs(grp.size() == 1 ? grp[0] : sum_refs(e_, grp.data(), grp.size()), LUT_MSG));
                grp.clear();
            };
            for (const Ref &b : blocks) {
                grp.push_back(b);
                if (grp.size() > 1 && var_of(grp) > 60) {     // b does not fit: close the group without it
                    grp.pop_back();
                    close();
                    grp.push_back(b);
                }
            }
            close();
            // A pass that merged nothing still REFRESHED every block (each was too noisy to share a group): the fresh
            // blocks merge in the next pass (64 refreshed blocks + 9 = 73 used to leave here un-merged).  Only
            // a second pass in a row without progress -- fresh blocks that are one shared node, say -- ends the loop.
            const bool stalled = nxt.size() >= blocks.size();
            blocks.swap(nxt);
            if (stalled && stalled_before) break;
            stalled_before = stalled;
        }
        Ref digit = blocks.empty() ? trivial_block(e_, 0) : (blocks.size() == 1 ? blocks[0] : sum_refs(e_, blocks.data(), blocks.size()));
        // 255 = 3,3,3,3 when absent.  The digit is a sum of at most 48 + 9 bootstrap-output variances, inside the budget of
        // one more bootstrap, and its value never leaves 0..3 (found: nf = 0; absent: every block is 0): it is handed back
        // as it is -- like a comparison's verdict -- instead of paying one more dependency level for a refresh; consumers
        // that weigh their operands refresh them by the engine's bookkeeping.
        r[d] = lin(e_, {{1, &digit}, {3, &nf}});
    }
    return r;
}

// Position encoded by one-hot flags: sum_i pick_i * (i + offset) digit-wise (at most one pick is set);
// when `absent_flag` is set the result is `absent_value` (255 for rfind, mod.rs:1023).
// Noise: a sum of k bootstrap outputs with weights c carries sum c^2 output variances into the next bootstrap, so
// the weighted picks are grouped by WEIGHT (sum of digit^2 <= FHS_NOISE_BUDGET_SUM_C2, not by count), every group is
// refreshed with LUT_MSG before groups are added up, and the digits handed back to the caller are refreshed too:
// like every op of the reference (fheasciichar.rs:35-104) the result is a fresh, clean-carry ciphertext.
// `digits` = 4: a u8 position; 8: a 16-bit one, absent_value up to 65535.
Strings::Num Strings::position_of(const std::vector<Ref> &pick, size_t off, const Ref *absent_flag, int absent_value,
                                  size_t digits) {
    const size_t W = pick.size();
    Num r(digits);
    // At most one pick is set.  A block that serves as the pick of TWO positions (mostly plaintext strings: one shared
    // bootstrap) can therefore never be set and is left out -- summed, its digits would add up to one large coefficient.
    std::vector<bool> twice(W, false);
    {
        std::vector<std::pair<Bid, size_t>> ids;
        ids.reserve(W);
        for (size_t i = 0; i < W; i++)
            if (!e_->is_triv(pick[i].id())) ids.push_back({pick[i].id(), i});
        std::sort(ids.begin(), ids.end());
        for (size_t a = 0; a + 1 < ids.size(); a++)
            if (ids[a].first == ids[a + 1].first) twice[ids[a].second] = twice[ids[a + 1].second] = true;
    }
    for (size_t blk = 0; blk < digits; blk++) {
        std::vector<Ref> cur;
        {
            Term tt[64];
            size_t m = 0;
            int64_t c2 = 0;
            // a lone group also takes the `absent` term (weight <= 3) before its refresh
            const int64_t limit = FHS_NOISE_BUDGET_SUM_C2 - (absent_flag ? 9 : 0);
            auto close = [&] {
                if (m) cur.push_back(Ref(e_, e_->lin(tt, m, 0)));
                m = 0;
                c2 = 0;
            };
            for (size_t i = 0; i < W; i++) {
                const int dig = (int)(((i + off) >> (2 * blk)) & 3);
                if (twice[i]) continue;
                if (!dig || e_->is_triv(pick[i].id())) {
                    if (dig && e_->triv_val(pick[i].id())) {                                    // folds into the constant
                        if (m == 64) close();               // tt is full: never write tt[64] (either branch may fill it)
                        tt[m++] = {dig, pick[i].id()};
                    }
                    continue;
                }
                if (c2 + dig * dig > limit || m == 64) close();
                tt[m++] = {dig, pick[i].id()};
                c2 += dig * dig;
            }
            close();
        }
        // tree of refreshed partial sums: <= 15 fresh digits (one-hot: the value stays <= 3) per node
        while (cur.size() > 1) {
            std::vector<Ref> nxt;
            for (size_t g = 0; g < cur.size(); g += 15) {
                std::vector<Ref> fresh;
                for (size_t i = g; i < std::min(cur.size(), g + 15); i++) fresh.push_back(pbs(cur[i], LUT_MSG));
                nxt.push_back(fresh.size() == 1 ? fresh[0] : sum_refs(e_, fresh.data(), fresh.size()));
            }
            cur.swap(nxt);
        }
        Ref digit = cur.empty() ? trivial_block(e_, 0) : cur[0];
        if (absent_flag) digit = lin(e_, {{1, &digit}, {(absent_value >> (2 * blk)) & 3, absent_flag}});
        r[blk] = pbs(digit, LUT_MSG);                        // folds when everything was trivial
    }
    return r;
}

// rfind (mod.rs:727-790) re-associated: the LAST matching window wins (the loop ascends and overwrites);
// `s` already carries the NUL pushed at :737
Strings::Num Strings::f_rfind_digits(const FStr &s, const FStr &pat, size_t digits) {
    if (pat.empty()) {                                      // :747-760: index after the last non-NUL char
        std::vector<Ref> nz(s.size());
        for (size_t i = 0; i < s.size(); i++) nz[i] = char_zero_test(s[i], false);
        std::vector<Ref> after = suffix_or(nz);
        std::vector<Ref> last(s.size());
        for (size_t i = 0; i < s.size(); i++) last[i] = pbs(lin(e_, {{2, &nz[i]}, {1, &after[i]}}), LUT_IS2);
        return position_of(last, 1, nullptr, 0, digits);
    }
    if (pat.size() > s.size()) return Num(digits, trivial_block(e_, 3));
    const size_t E = std::max<size_t>(1, s.size() - pat.size());   // adjust_end_of_pattern, exclusive bound (:768-771)
    std::vector<Ref> f(E);
    for (size_t i = 0; i < E; i++) f[i] = window_match(s, i, pat);
    std::vector<Ref> after = suffix_or(f);
    std::vector<Ref> last(E);
    for (size_t i = 0; i < E; i++) last[i] = pbs(lin(e_, {{2, &f[i]}, {1, &after[i]}}), LUT_IS2);
    Ref found = or_tree(f);
    Ref nf = flag_not(found);
    return position_of(last, 0, &nf, (int)absent_value(digits / 4), digits);
}

// sum of 0/1 flags mod 4^digits: groups of 15 -> (low, high) digit pair, then 4-operand radix adds.
// With 8 digits the carry runs on through digits 4 to 7 (a carry out of digit 7 needs 65536 flags), but
// only as far as a partial sum can reach: a digit above the largest possible value stays a trivial 0 instead of two
// bootstraps on a carry that is always 0.  The four low digits are always computed, as the u8 form has them.
Strings::Num Strings::count_flags(const std::vector<Ref> &flags, size_t digits) {
    std::vector<Num> nums;
    std::vector<size_t> most;                                // the largest value each partial sum can take
    for (size_t i = 0; i < flags.size(); i += 15) {
        const size_t n = std::min<size_t>(15, flags.size() - i);
        Ref s = sum_refs(e_, &flags[i], n);
        Num c(digits);
        if (e_->sum_c2(s.id()) > FHS_NOISE_BUDGET_SUM_C2) {  // the same flag many times over (`repeat`): count in halves
            Num v = count_digits(&flags[i], n, 2);
            c[0] = v[0];
            c[1] = v[1];
        } else {
            c[0] = pbs(s, LUT_MSG);
            c[1] = n >= 4 ? pbs(s, LUT_CARRY) : trivial_block(e_, 0);
        }
        for (size_t d = 2; d < digits; d++) c[d] = trivial_block(e_, 0);
        nums.push_back(c);
        most.push_back(n);
    }
    if (nums.empty()) return Num(digits, trivial_block(e_, 0));
    while (nums.size() > 1) {
        std::vector<Num> nxt;
        std::vector<size_t> nxt_most;
        for (size_t i = 0; i < nums.size(); i += 4) {
            const size_t n = std::min<size_t>(4, nums.size() - i);
            size_t top = 0;
            for (size_t u = 0; u < n; u++) top += most[i + u];
            nxt_most.push_back(top);
            if (n == 1) { nxt.push_back(nums[i]); continue; }
            size_t live = 4;
            while (live < digits && (top >> (2 * live)) != 0) live++;
            Num r(digits, trivial_block(e_, 0));
            Ref carry;
            for (size_t blk = 0; blk < std::min(live, digits); blk++) {
                Term tt[8];
                size_t k = 0;
                for (size_t u = 0; u < n; u++) tt[k++] = {1, nums[i + u][blk].id()};
                if (carry) tt[k++] = {1, carry.id()};
                Ref sm(e_, e_->lin(tt, k, 0));   // <= 4*3 + 3 = 15
                r[blk] = pbs(sm, LUT_MSG);
                if (blk + 1 < std::min(live, digits)) carry = pbs(sm, LUT_CARRY);
            }
            nxt.push_back(r);
        }
        nums.swap(nxt);
        most.swap(nxt_most);
    }
    return nums[0];
}

// ---------------------------------------------------------------------------------------------
// encrypted positions as operands: char_at, substr, take, split_at.  The reference has no such
// method -- its positions are only ever decrypted.  A position is what find / rfind / len return, one half or two; its
// value is taken literally as an index into the buffer, NULs and all.
// ---------------------------------------------------------------------------------------------
FChar Strings::char_at(const FStr &s, const Pos &pos) { return substr(s, pos, 1)[0]; }
void Strings::split_at(const FStr &s, const Pos &pos, FStr *head, FStr *tail) {
    *head = take(s, pos);                                    // the bits of the shift are those the thermometer's digits
    *tail = substr(s, pos, s.size());                        // came from: one refresh, found again by the engine
}

// as written: the position against a clear index with the char operators, the wide form from its two halves
FChar Strings::pos_eq(const Pos &pos, size_t i) {
    FChar r = ch_eq(pos[0], t((uint8_t)(i & 255)));
    if (pos.size() > 1) r = ch_bitand(r, ch_eq(pos[1], t((uint8_t)(i >> 8))));
    return r;
}
FChar Strings::pos_gt(const Pos &pos, size_t j) {
    if (pos.size() == 1) return ch_gt(pos[0], t((uint8_t)j));
    const FChar jl = t((uint8_t)(j & 255)), jh = t((uint8_t)(j >> 8));
    return ch_bitor(ch_gt(pos[1], jh), ch_bitand(ch_eq(pos[1], jh), ch_gt(pos[0], jl)));
}

FStr Strings::substr(const FStr &s, const Pos &pos, size_t count) {
    const size_t n = s.size();
    FStr out(count, t(0));
    if (n == 0 || count == 0) return out;
    if (fused()) return f_pos_shift(s, pos_digits(pos), count);
    const size_t reach = std::min(n, (size_t)1 << (8 * pos.size()));   // indices the position can name
    for (size_t i = 0; i < reach; i++) {
        FChar hit = pos_eq(pos, i);
        for (size_t j = 0; j < count && i + j < n; j++) out[j] = ch_ite(hit, s[i + j], out[j]);
    }
    return out;
}

FStr Strings::take(const FStr &s, const Pos &pos) {
    const size_t n = s.size();
    if (n == 0) return {};
    if (fused()) return f_pos_take(s, pos_digits(pos));
    const size_t reach = std::min(n, (size_t)1 << (8 * pos.size()));
    const FChar zero = t(0);
    FStr out(n, zero);
    for (size_t j = 0; j < reach; j++) out[j] = ch_ite(pos_gt(pos, j), s[j], zero);
    return out;
}

// The digits of a position, least significant first.  find's index digits are sums of up to 57 bootstrap outputs; they
// enter the selects below with other blocks beside them, so anything above 4 is refreshed first (what loading an
// operand over the C ABI does as well).
Strings::Num Strings::pos_digits(const Pos &pos) {
    Num dg;
    for (const FChar &c : pos)
        for (int k = 0; k < 4; k++) dg.push_back(e_->sum_c2(c.b[k].id()) > 4 ? pbs(c.b[k], LUT_MSG) : c.b[k]);
    return dg;
}

// Bit k of the position from digit k / 2 (one bootstrap each), for the K bits a shift on n characters can use
// (2^K >= n, at most all of them), and ONE flag for everything above: the non-zero test on the sum of the higher digits
// -- five to a bootstrap, 15 at most -- and on bit K itself where K is odd.  A trivial digit folds.
Strings::PosBits Strings::f_pos_bits(const Num &dg, size_t n) {
    PosBits pb;
    const int B = 2 * (int)dg.size();
    while (pb.K < B && ((size_t)1 << pb.K) < n) pb.K++;
    for (int k = 0; k < pb.K; k++) pb.bit.push_back(pbs(dg[k / 2], (k & 1) ? LUT_BIT1_UNLESS : LUT_BIT0_UNLESS));
    std::vector<Ref> high;
    if (pb.K & 1) high.push_back(pbs(dg[pb.K / 2], LUT_BIT1_UNLESS));
    for (size_t q = ((size_t)pb.K + 1) / 2; q < dg.size(); q += 5)
        high.push_back(pbs(sum_refs(e_, &dg[q], std::min<size_t>(5, dg.size() - q)), LUT_NZ));
    pb.ovf = or_tree(high);
    return pb;
}

// out[j] = s[p + j] (0 past the end), j < count: the shift by an encrypted amount that is the same for every character.
// A stage moves by 2^k where bit k of p is set, f_compact's rule with one move flag for the whole stage:
//     m[i] = bit_k ? cur[i] : 0 (one bootstrap per block),    next[i] = cur[i] - m[i] + m[i + 2^k]   (exact, linear).
// One shift for all has no collisions to avoid, so the stages may run in either order of the bits, and only what an
// output can still be reached from is computed: stage t works on need[t] = need[t+1] u (need[t+1] + 2^k), pruned
// backwards from the outputs.  From the highest bit down, what is left to shift by after bit k is below 2^k and only the
// first 2^k + count - 1 characters matter: n + K count characters in all instead of n K, but up to 3 n for one character
// of a buffer just above a power of two.  From the lowest bit up the working set halves with every stage: 2 n for one
// character, about n log2(n / count) + n for `count`.  Both are counted and the cheaper order is recorded, so char_at
// (count 1) is linear in n.  A stage whose bit is trivial is a static shift.  After t stages a block is a sum of its
// operand (sum c^2 <= 4) and 2 t bootstrap outputs; the select's input carries 16 + 4 + 2 t <= 50.  The last bootstrap
// refreshes the result and, with the overflow flag at weight 4, turns it into NUL when the position has a bit the stages
// did not use.
FStr Strings::f_pos_shift(const FStr &s, const Num &dg, size_t count) {
    const size_t n = s.size();
    const PosBits pb = f_pos_bits(dg, n);
    const int K = pb.K;
    const Ref zero = trivial_block(e_, 0);
    auto is_zero = [&](const Ref &r) { return e_->is_triv(r.id()) && e_->triv_val(r.id()) == 0; };
    // need[t][i]: character i is still wanted before stage t, which uses bit (down ? K - 1 - t : t); returns the selects
    std::vector<std::vector<char>> need;
    auto plan = [&](bool down) {
        need.assign((size_t)K + 1, std::vector<char>(n, 0));
        for (size_t j = 0; j < std::min(count, n); j++) need[K][j] = 1;
        size_t selects = 0;
        for (int t = K; t-- > 0;) {
            const size_t d = (size_t)1 << (down ? K - 1 - t : t);
            for (size_t i = 0; i < n; i++)
                if (need[t + 1][i]) {
                    need[t][i] = 1;
                    if (i + d < n) need[t][i + d] = 1;
                }
            for (size_t i = 0; i < n; i++) selects += need[t][i];
        }
        return selects;
    };
    const size_t cost_up = plan(false);
    const bool down = plan(true) <= cost_up;
    if (!down) plan(false);
    FStr cur = s;
    for (int t = 0; t < K; t++) {
        const int k = down ? K - 1 - t : t;
        const size_t d = (size_t)1 << k;
        const Ref &bit = pb.bit[k];
        if (is_zero(bit)) continue;
        FStr nxt(n);
        if (e_->is_triv(bit.id())) {                         // a clear 1: everything moves
            for (size_t i = 0; i < n; i++)
                if (need[t + 1][i])
                    for (int blk = 0; blk < 4; blk++) nxt[i].b[blk] = i + d < n ? cur[i + d].b[blk] : zero;
            cur.swap(nxt);
            continue;
        }
        FStr m(n);
        for (size_t i = 0; i < n; i++)
            if (need[t][i])
                for (int blk = 0; blk < 4; blk++)
                    m[i].b[blk] = is_zero(cur[i].b[blk]) ? zero : pbs(lin(e_, {{4, &bit}, {1, &cur[i].b[blk]}}), LUT_SEL_T);
        for (size_t i = 0; i < n; i++)
            if (need[t + 1][i])
                for (int blk = 0; blk < 4; blk++)
                    nxt[i].b[blk] = lin(e_, {{1, &cur[i].b[blk]}, {-1, &m[i].b[blk]}, {1, i + d < n ? &m[i + d].b[blk] : &zero}});
        cur.swap(nxt);
    }
    const bool ovf_clear = e_->is_triv(pb.ovf.id());
    FStr out(count);
    for (size_t j = 0; j < count; j++)
        for (int blk = 0; blk < 4; blk++) {
            Ref &o = out[j].b[blk];
            if (j >= n || is_zero(cur[j].b[blk]) || (ovf_clear && !is_zero(pb.ovf))) o = zero;
            else if (!ovf_clear) o = pbs(lin(e_, {{4, &pb.ovf}, {1, &cur[j].b[blk]}}), LUT_SEL_F);
            else o = e_->sum_c2(cur[j].b[blk].id()) > 4 ? pbs(cur[j].b[blk], LUT_MSG) : cur[j].b[blk];
        }
    return out;
}

// g[j] = [p > j] for j < limit, from the digits most significant first.  Every clear prefix of q digits carries the
// three-state comparison s of the position's top q digits with it (0 below, 1 equal, 2 above; the empty prefix: equal),
// and one bootstrap on 4 s + digit - c takes it one digit further down for the clear digit c (LUT_POS_CMP; LUT_POS_GT
// at the last digit, where only "above" is asked).  The four children of a prefix differ in the constant c alone: they
// are extractions of one blind rotation, so the tree of limit + limit / 4 + ... nodes costs about limit / 3 rotations.
// Prefixes no index below `limit` has are not built.  Inputs carry 16 + 4.
std::vector<Ref> Strings::f_pos_thermometer(const Num &dg, size_t limit) {
    std::vector<Ref> state{trivial_block(e_, 1)};
    for (size_t q = dg.size(); q-- > 0;) {
        const size_t S = (size_t)1 << (2 * q), count = (limit + S - 1) / S;
        std::vector<Ref> nxt(count);
        for (size_t p = 0; p < count; p++)
            nxt[p] = pbs(lin(e_, {{4, &state[p / 4]}, {1, &dg[q]}}, -(int)(p % 4)), q ? LUT_POS_CMP : LUT_POS_GT);
        state.swap(nxt);
    }
    return state;
}

// take[j] = g[j] ? s[j] : 0, one select per block (16 + 4).  An index no value of the position exceeds (j >= 4^digits:
// a u8 position on a long buffer) is a clear NUL.
FStr Strings::f_pos_take(const FStr &s, const Num &dg) {
    const size_t n = s.size(), limit = std::min(n, (size_t)1 << (2 * dg.size()));
    const std::vector<Ref> g = f_pos_thermometer(dg, limit);
    const Ref zero = trivial_block(e_, 0);
    FStr out(n);
    for (size_t j = 0; j < n; j++)
        for (int blk = 0; blk < 4; blk++) {
            const Ref &x = s[j].b[blk];
            Ref &o = out[j].b[blk];
            if (j >= limit || (e_->is_triv(x.id()) && e_->triv_val(x.id()) == 0)) o = zero;
            else if (e_->is_triv(g[j].id())) o = e_->triv_val(g[j].id()) ? x : zero;
            else o = pbs(lin(e_, {{4, &g[j]}, {1, &x}}), LUT_SEL_T);
        }
    return out;
}

}  // namespace fhs
