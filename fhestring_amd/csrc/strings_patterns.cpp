// String layer, part 7 of 7: LIKE and regular expressions against clear patterns.
#include "strings.h"

#include <algorithm>
#include <cstring>
#include <set>

#include "strings_internal.h"

namespace fhs {

// ---------------------------------------------------------------------------------------------
// LIKE against a clear pattern.  The reference has no such method; the semantics are those of
//     re.match(rb'\A' + body + rb'(?=\x00|\Z)', buf, re.S [| re.I])
// with body = [\x00-\xff]* for ANY, [^\x00] for ONE and the escaped byte for a literal, on the buffer as it is.
// ---------------------------------------------------------------------------------------------
bool Strings::like_parse(const char *pat, size_t m, int escape, std::vector<LikeTok> *out) {
    if (escape != -1 && (escape <= 0 || escape > 255 || escape == '%' || escape == '_')) return false;
    out->clear();
    for (size_t i = 0; i < m; i++) {
        const uint8_t c = (uint8_t)pat[i];
        if (c == 0) return false;
        if ((int)c == escape) {                              // e%, e_ and ee are the literals %, _ and e
            const uint8_t d = i + 1 < m ? (uint8_t)pat[++i] : 0;
            if (d != '%' && d != '_' && (int)d != escape) return false;
            out->push_back({LikeTok::LIT, d});
        } else if (c == '%') out->push_back({LikeTok::ANY, 0});
        else if (c == '_') out->push_back({LikeTok::ONE, 0});
        else out->push_back({LikeTok::LIT, c});
    }
    return true;
}

int Strings::like_trivial(const std::vector<LikeTok> &pat, size_t n) {
    size_t fixed = 0;
    for (const LikeTok &k : pat) fixed += k.kind != LikeTok::ANY;
    if (fixed > n) return 0;
    return fixed == 0 && !pat.empty() ? 1 : -1;
}

static bool ascii_letter(uint8_t c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }

FChar Strings::like(const FStr &s, const std::vector<LikeTok> &pat, bool ignore_case) {
    const int k = like_trivial(pat, s.size());
    if (k >= 0) return t((uint8_t)k);
    return fused() ? f_like(s, pat, ignore_case) : like_as_written(s, pat, ignore_case);
}

// The as-written 0/1-flag algebra of LIKE and of the regular expressions.  A flag that is a trivial constant is not sent
// through a bitand / bitor: x & 1 = x, x & 0 = 0, x | 0 = x, x | 1 = 1.  That also keeps what the shape alone decides --
// an automaton position that cannot be reached after i + 1 characters, or cannot end a match in the characters that are
// left -- free of charge.
int Strings::flag_const(const FChar &f) const {              // 0 / 1 for a trivial flag, -1 for an encrypted one
    int v = 0;
    for (int k = 0; k < 4; k++) {
        if (!e_->is_triv(f.b[k].id())) return -1;
        v |= (e_->triv_val(f.b[k].id()) & 3) << (2 * k);
    }
    return v;
}
FChar Strings::flag_and(const FChar &a, const FChar &b) {
    const int ka = flag_const(a), kb = flag_const(b);
    if (ka == 0 || kb == 0) return t(0);
    if (ka == 1) return b;
    if (kb == 1) return a;
    return ch_bitand(a, b);
}
FChar Strings::flag_or(const FChar &a, const FChar &b) {
    const int ka = flag_const(a), kb = flag_const(b);
    if (ka == 1 || kb == 1) return t(1);
    if (ka == 0) return b;
    if (kb == 0) return a;
    return ch_bitor(a, b);
}
FChar Strings::any_of(const std::vector<FChar> &flags, uint64_t set) {   // OR of the flags whose index is in the set
    FChar r = t(0);
    for (size_t p = 0; p < flags.size(); p++)
        if ((set >> p) & 1) r = flag_or(r, flags[p]);
    return r;
}
// [c in cls] as the OR over the class's runs of consecutive bytes of eq (one byte), ne 0 (every byte), ge, or ge & le
FChar Strings::class_test_as_written(const FChar &c, const RegexClass &cls) {
    const FChar zero = t(0);
    FChar f = zero;
    for (int lo = 1; lo < 256; lo++) {
        if (!cls.has(lo)) continue;
        int hi = lo;
        while (hi < 255 && cls.has(hi + 1)) hi++;
        FChar run;
        if (lo == hi) run = ch_eq(c, t((uint8_t)lo));
        else if (lo == 1 && hi == 255) run = ch_ne(c, zero);
        else {
            run = ch_ge(c, t((uint8_t)lo));                  // recorded before the le
            if (hi < 255) run = flag_and(run, ch_le(c, t((uint8_t)hi)));
        }
        f = flag_or(f, run);
        lo = hi;
    }
    return f;
}

// As written: the textbook dynamic programme, one row per token.  reach[j][i] = the first j tokens match the first i
// characters; LIT: reach[j-1][i-1] & eq(s[i-1], c) (either case OR-ed under ignore_case, the pattern's first), ONE:
// reach[j-1][i-1] & ne(s[i-1], 0), ANY: reach[j-1][i] | reach[j][i-1]; result OR_i reach[m][i] & end[i], end[i] = (i == n)
// | eq(s[i], 0).  A test of one character against one byte is made once.
FChar Strings::like_as_written(const FStr &s, const std::vector<LikeTok> &pat, bool ignore_case) {
    const size_t n = s.size();
    const FChar zero = t(0), one = t(1);
    std::vector<std::vector<std::pair<int, FChar>>> tests(n);   // per character: (byte, eq(s[i], byte)); -1: ne(s[i], 0)
    auto test = [&](size_t i, int c) {
        for (const auto &kv : tests[i])
            if (kv.first == c) return kv.second;
        tests[i].emplace_back(c, c < 0 ? ch_ne(s[i], zero) : ch_eq(s[i], t((uint8_t)c)));
        return tests[i].back().second;
    };
    std::vector<FChar> prev(n + 1, zero), cur(n + 1, zero);
    prev[0] = one;
    for (const LikeTok &k : pat) {
        if (k.kind == LikeTok::ANY) {
            cur[0] = prev[0];
            for (size_t i = 1; i <= n; i++) cur[i] = flag_or(prev[i], cur[i - 1]);
        } else {
            cur[0] = zero;
            for (size_t i = 1; i <= n; i++) {
                if (flag_const(prev[i - 1]) == 0) { cur[i] = zero; continue; }
                FChar hit = k.kind == LikeTok::ONE ? test(i - 1, -1) : test(i - 1, k.c);
                if (k.kind == LikeTok::LIT && ignore_case && ascii_letter(k.c)) hit = flag_or(hit, test(i - 1, k.c ^ 0x20));
                cur[i] = flag_and(prev[i - 1], hit);
            }
        }
        prev.swap(cur);
    }
    FChar result = zero;
    for (size_t i = 0; i <= n; i++) {
        if (flag_const(prev[i]) == 0) continue;
        result = flag_or(result, flag_and(prev[i], i == n ? one : test(i, 0)));
    }
    return result;
}

// Fused: the tokens split at ANY into segments.  A segment's window flag at i is window_match's AND over the nibble tests
// of its literals -- is0(nibble - c) against any number of clear c is one blind rotation per nibble (rotation sharing), so
// every segment of every pattern rides on the 2 n rotations contains_clear runs -- with the shared per-character flag
// nz[i] = [s[i] != 0] for a ONE.  Segment k can END at lo_k + L_k + w (lo_k = the lengths before it, w < W = n - all
// lengths + 1: further right the rest would not fit) iff its window there matches and the segment before it can end at
// or before its start: E_k[w] = M_k[lo_k + w] & A_k[w], A_k = inclusive prefix OR of E_{k-1}; A_k[w] joins the last level
// of the window's AND instead of a bootstrap of its own.  The first segment is tested at 0 only (no leading ANY), or A is
// trivially 1 (and_tree drops it); the last one also carries end[j] = 1 - nz[j] (j < n; end[n] = 1) unless the pattern
// ends in ANY, where the result is the OR of the last segment's flags: '%lit%' records what contains_clear(lit) records.
// ignore_case: byte_eq_flags' high-nibble flag of a letter carries sum c^2 = 4 -- an AND of 15 flags holds at most 8 of
// them: 8 * 4 + 7 = 39 of the budget of 64.
FChar Strings::f_like(const FStr &s, const std::vector<LikeTok> &pat, bool ignore_case) {
    const size_t n = s.size();
    const Ref one = trivial_block(e_, 1);
    std::vector<std::vector<LikeTok>> seg(1);
    size_t fixed = 0;
    for (const LikeTok &k : pat) {
        if (k.kind == LikeTok::ANY) seg.emplace_back();
        else { seg.back().push_back(k); fixed++; }
    }
    NzMemo nz(this, s);
    auto end_at = [&](size_t j) { return j == n ? one : nz.zero(j); };
    // AND of a window's flags and of `extra` (the flags that come from deeper in the DAG: they join the tree's last level)
    auto window = [&](const std::vector<LikeTok> &sg, size_t at, std::vector<Ref> extra) {
        if (!drop_trivial(extra, 0)) return trivial_block(e_, 0);
        std::vector<Ref> f;
        for (size_t j = 0; j < sg.size(); j++) {
            if (sg[j].kind == LikeTok::ONE) { f.push_back(nz(at + j)); continue; }
            for (const Ref &x : byte_eq_flags(s[at + j], sg[j].c, ignore_case && ascii_letter(sg[j].c))) f.push_back(x);
        }
        if (extra.empty()) return and_tree(f);
        while (f.size() + extra.size() > 15) {
            std::vector<Ref> nxt;
            for (size_t i = 0; i < f.size(); i += 15)
                nxt.push_back(and_tree(std::vector<Ref>(f.begin() + i, f.begin() + std::min(i + 15, f.size()))));
            f.swap(nxt);
        }
        f.insert(f.end(), extra.begin(), extra.end());
        return and_tree(f);
    };
    if (seg.size() == 1)                                     // no ANY: one segment, anchored at both ends
        return ch_flag(e_, window(seg[0], 0, {end_at(fixed)}));
    const size_t W = n - fixed + 1;
    auto inclusive_or = [&](std::vector<Ref> f) {            // prefix_or is exclusive: one more (unused) flag behind
        f.push_back(trivial_block(e_, 0));
        const std::vector<Ref> p = prefix_or(f);
        return std::vector<Ref>(p.begin() + 1, p.end());
    };
    std::vector<Ref> E, A;                                   // E: where the last segment done can end; A: made from E on demand
    size_t lo = seg[0].size();
    if (seg[0].empty()) A.assign(W, one);
    else {
        E.assign(1, window(seg[0], 0, {}));
        A.assign(W, E[0]);
    }
    bool a_ready = true;
    for (size_t k = 1; k + 1 < seg.size(); k++) {
        if (seg[k].empty()) continue;                        // adjacent ANYs
        if (!a_ready) A = inclusive_or(E);
        E.resize(W);
        for (size_t w = 0; w < W; w++) E[w] = window(seg[k], lo + w, {A[w]});
        lo += seg[k].size();
        a_ready = false;
    }
    const std::vector<LikeTok> &last = seg.back();
    if (last.empty()) return ch_flag(e_, or_tree(E));        // fixed > 0: some segment has been done
    if (!a_ready) A = inclusive_or(E);
    std::vector<Ref> R(W);
    for (size_t w = 0; w < W; w++) R[w] = window(last, lo + w, {A[w], end_at(lo + w + last.size())});
    return ch_flag(e_, or_tree(R));
}

// ---------------------------------------------------------------------------------------------
// Regular expressions against a clear pattern.  The reference has no such method; the semantics
// are re.fullmatch(pat, text, re.S [| re.I]) -- re.search with FHS_REGEX_SEARCH, compiled as .*(?:pat).* -- on text =
// the buffer up to its first NUL.  No atom matches NUL, so on the buffer the condition is LIKE's: the match starts at 0
// and ends at j with j == n or s[j] == NUL.  The pattern arrives as its position automaton (regex.h): every edge into a
// position q reads q's class, so one flag per (position, index) is all the state there is:
//     act[q][i] = in_q(s[i]) & (OR_{p in pred(q)} act[p][i-1]  |  q in first, i == 0)
//     result    = OR_j end[j] & OR_{q in last} act[q][j-1]   (+ end[0] if nullable),  end[j] = [s[j] == 0], end[n] = 1
// ---------------------------------------------------------------------------------------------
int Strings::regex_trivial(const RegexProgram &g, size_t n) {
    if (g.min_len > n) return 0;
    if (n == 0) return 1;                                    // the empty text and a nullable pattern
    return g.matches_everything() ? 1 : -1;
}

bool Strings::regex_plan(const RegexProgram &g, RegexPlan *out) {
    const size_t K = g.classes.size();
    out->kind.assign(K, RegexPlan::TABLE);
    out->byte.assign(K, 0);
    out->both_cases.assign(K, 0);
    out->table.assign(K, TablePlan());
    for (size_t k = 0; k < K; k++) {
        const RegexClass &c = g.classes[k];
        const int members = c.count();
        int lowest = 0;
        while (lowest < 255 && !c.has(lowest)) lowest++;
        if (members == 0) out->kind[k] = RegexPlan::DEAD;
        else if (members == 255) out->kind[k] = RegexPlan::ANY;
        else if (members == 1 || (members == 2 && lowest >= 'A' && lowest <= 'Z' && c.has(lowest | 0x20))) {
            out->kind[k] = RegexPlan::BYTE;
            out->byte[k] = (uint8_t)lowest;
            out->both_cases[k] = members == 2;
        } else if (!plan_class(c.bits, &out->table[k])) return false;    // (as written: the set only, nothing is registered)
    }
    if (!fused()) return true;
    // Every threshold table regex_step can ask for is registered here, before an operand is loaded, so that a full
    // registry fails with nothing recorded: a step with k >= 2 of a position's predecessors (an end: of the last
    // positions) and u class flags, u = 2 nibble flags for a BYTE class of which one may fold away.
    auto thresholds = [&](int preds, int flags) {
        for (int k = 2; k <= preds; k++)
            for (int u = 1; u <= flags; u++) {
                const int w = k + 1;
                if (w * u + k > 15) continue;                 // or_tree first, then one predecessor: an is-k table
                uint8_t values[16];
                for (int v = 0; v < 16; v++) values[v] = v >= w * u + 1;
                if (user_table(values) < 0) return false;
            }
        return true;
    };
    int last = 0;
    for (size_t q = 0; q < g.positions(); q++) {
        int preds = 0;
        for (size_t p = 0; p < g.positions(); p++) preds += (int)((g.pred[q] >> p) & 1);
        last += (int)((g.last >> q) & 1);
        if (!thresholds(preds, out->kind[g.cls[q]] == RegexPlan::BYTE ? 2 : 1)) return false;
    }
    return thresholds(last, 1);
}

FChar Strings::regex(const FStr &s, const RegexProgram &g, const RegexPlan &plan) {
    const int k = regex_trivial(g, s.size());
    if (k >= 0) return t((uint8_t)k);
    return fused() ? f_regex(s, g, plan) : regex_as_written(s, g);
}

// As written: exactly the recurrence above from char operations and the as-written flag algebra (flag_and, flag_or,
// any_of, class_test_as_written); a test of one character against one class is made once.
FChar Strings::regex_as_written(const FStr &s, const RegexProgram &g) {
    const size_t n = s.size(), P = g.positions();
    const FChar zero = t(0), one = t(1);
    std::vector<FStr> tests(g.classes.size(), FStr(n));      // [class][index]
    auto test = [&](size_t k, size_t i) {
        if (!tests[k][i].b[0]) tests[k][i] = class_test_as_written(s[i], g.classes[k]);
        return tests[k][i];
    };
    FChar result = !g.nullable ? zero : (n ? ch_eq(s[0], zero) : one);
    std::vector<FChar> prev(P, zero), cur(P, zero);
    for (size_t i = 0; i < n; i++) {
        for (size_t q = 0; q < P; q++) {
            const FChar before = i == 0 ? (((g.first >> q) & 1) ? one : zero) : any_of(prev, g.pred[q]);
            cur[q] = flag_const(before) == 0 ? zero : flag_and(test((size_t)g.cls[q], i), before);
        }
        const FChar ended = any_of(cur, g.last);             // every end[j] is asked for once
        if (flag_const(ended) != 0) result = flag_or(result, flag_and(ended, i + 1 == n ? one : ch_eq(s[i + 1], zero)));
        prev.swap(cur);
    }
    return result;
}

// d[q] = the fewest characters from position q to a position of `from` along the edges `towards` (0: q is one of them),
// FAR if there is no way; a position whose class is dead lies on no way.
static const size_t FAR = (size_t)-1;
static std::vector<size_t> regex_distances(const RegexProgram &g, const Strings::RegexPlan &plan, uint64_t from,
                                           const std::vector<uint64_t> &towards) {
    const size_t P = g.positions();
    auto alive = [&](size_t q) { return plan.kind[g.cls[q]] != Strings::RegexPlan::DEAD; };
    std::vector<size_t> d(P, FAR);
    for (size_t q = 0; q < P; q++)
        if (((from >> q) & 1) && alive(q)) d[q] = 0;
    for (size_t round = 0; round < P; round++)
        for (size_t q = 0; q < P; q++)
            for (size_t p = 0; p < P; p++)
                if (((towards[q] >> p) & 1) && d[p] != FAR && alive(q)) d[q] = std::min(d[q], d[p] + 1);
    return d;
}

// AND of the 0/1 flags `in` (at most two) AND the OR of the 0/1 flags `preds`, in ONE bootstrap where the noise budget
// and the message space allow: with k predecessors the input is w * sum(in) + sum(preds), w = k + 1, which exceeds
// w * |in| exactly when every `in` flag and at least one predecessor is set -- a threshold table (a user table; with one
// predecessor the threshold is the largest value and the catalogue's is-k table does).  More predecessors than that go
// through or_tree first.  Trivial flags fold.
Ref Strings::regex_step(std::vector<Ref> in, std::vector<Ref> preds_all) {
    const Ref zero = trivial_block(e_, 0);
    if (!drop_trivial(in, 0)) return zero;
    std::vector<Ref> preds;
    if (drop_trivial(preds_all, 1)) {                        // (a trivial 1 among them: the OR is satisfied, none is left)
        for (const Ref &x : preds_all) {
            bool seen = false;                               // positions with one class and one history are one block
            for (const Ref &y : preds) seen = seen || y.id() == x.id();
            if (!seen) preds.push_back(x);
        }
        if (preds.empty()) return zero;
    }
    if (in.empty()) return preds.empty() ? trivial_block(e_, 1) : or_tree(preds);
    if (preds.empty()) return in.size() == 1 ? in[0] : and_tree(in);
    for (;;) {
        const int k = (int)preds.size(), u = (int)in.size(), w = k + 1;
        std::vector<Term> tt;
        for (const Ref &x : in) tt.push_back({w, x.id()});
        for (const Ref &x : preds) tt.push_back({1, x.id()});
        const Ref d(e_, e_->lin(tt.data(), tt.size(), 0));
        const int top = w * u + k, threshold = w * u + 1;
        if (top <= 15 && e_->sum_c2(d.id()) <= FHS_NOISE_BUDGET_SUM_C2) {
            if (threshold == top) return pbs(d, lut_is_k(top));
            uint8_t values[16];
            for (int v = 0; v < 16; v++) values[v] = v >= threshold;
            const int lut = user_table(values);              // registered by regex_plan: the interned id, cannot fail
            return lut < 0 ? zero : pbs(d, lut);
        }
        if (k > 1) { preds.assign(1, or_tree(preds)); continue; }
        for (Ref &x : in)                                     // one predecessor and still too much: refresh what is a sum
            if (e_->sum_c2(x.id()) > 1) x = pbs(x, LUT_NZ);
        if (e_->sum_c2(preds[0].id()) > 1) preds[0] = pbs(preds[0], LUT_NZ);
    }
}

std::vector<std::vector<std::vector<Ref>>> Strings::regex_class_tests(const FStr &s, const RegexProgram &g, const RegexPlan &plan,
                                                                      const std::vector<uint64_t> &live, NzMemo &nz) {
    const size_t n = s.size(), P = g.positions(), K = g.classes.size();
    std::vector<std::vector<std::vector<Ref>>> in(K, std::vector<std::vector<Ref>>(n));
    for (size_t k = 0; k < K; k++) {
        std::vector<size_t> where;
        for (size_t i = 0; i < n; i++)
            for (size_t q = 0; q < P; q++)
                if (((live[i] >> q) & 1) && (size_t)g.cls[q] == k) { where.push_back(i); break; }
        if (plan.kind[k] == RegexPlan::TABLE) {
            FStr sub;
            for (size_t i : where) sub.push_back(s[i]);
            const std::vector<Ref> f = f_class_flags(sub, plan.table[k]);
            for (size_t j = 0; j < where.size(); j++) in[k][where[j]].assign(1, f[j]);
            continue;
        }
        for (size_t i : where) {
            if (plan.kind[k] == RegexPlan::ANY) in[k][i].assign(1, nz(i));
            else in[k][i] = byte_eq_flags(s[i], plan.byte[k], plan.both_cases[k]);   // (the byte is the upper case)
        }
    }
    return in;
}

// Fused.  (1) The class tests of all characters stand at the front of the DAG: a class of one byte (or of the two cases
// of one letter) is the two nibble flags of block_eq_flags -- extractions of the two rotations per character that
// contains_clear and like_clear run, the other case's high nibble a second extraction summed to the first as in f_like
// -- every character is the shared nz flag, and any other class is f_class_flags of its TablePlan on the characters where
// a position of that class is live.  (2) One regex_step per live (q, i).  (3) (q, i) is live iff q can be reached after
// exactly i + 1 characters and some last position is at most n - i - 1 characters away from q: a literal of length L
// costs L steps on any n.  (4) The result is the or_tree over the ends: for j < n one regex_step of end[j] = 1 - nz[j]
// with the last positions live at j - 1, for j == n those flags themselves; nz[j] is made only where an end can fall.
FChar Strings::f_regex(const FStr &s, const RegexProgram &g, const RegexPlan &plan) {
    const size_t n = s.size(), P = g.positions();
    const Ref one = trivial_block(e_, 1);
    const std::vector<size_t> dist = regex_distances(g, plan, g.last, g.follow);   // from q to the nearest last position
    std::vector<uint64_t> live(n, 0);
    uint64_t reach = g.first;
    for (size_t i = 0; i < n; i++) {
        uint64_t next = 0;
        for (size_t q = 0; q < P; q++)
            if (((reach >> q) & 1) && dist[q] != FAR && dist[q] <= n - i - 1) {
                live[i] |= (uint64_t)1 << q;
                next |= g.follow[q];
            }
        reach = next;
    }
    NzMemo nz(this, s);
    // (1) class tests: in[k][i] holds one flag, or the two nibble flags of a BYTE class
    const std::vector<std::vector<std::vector<Ref>>> in = regex_class_tests(s, g, plan, live, nz);
    // (2) the steps; positions with the same live predecessors share the OR (the engine finds the same bootstrap again)
    std::vector<Ref> fin;
    if (g.nullable) fin.push_back(nz.zero(0));               // n > 0: the empty text is decided by regex_trivial otherwise
    std::vector<Ref> prev(P), cur(P);
    for (size_t i = 0; i < n && !err.code; i++) {
        std::vector<Ref> ended;
        for (size_t q = 0; q < P; q++) {
            cur[q] = Ref();
            if (!((live[i] >> q) & 1)) continue;
            std::vector<Ref> preds;
            if (i == 0) preds.push_back(one);
            else
                for (size_t p = 0; p < P; p++)
                    if (((g.pred[q] >> p) & 1) && prev[p]) preds.push_back(prev[p]);
            cur[q] = regex_step(in[g.cls[q]][i], preds);
            if ((g.last >> q) & 1) ended.push_back(cur[q]);
        }
        if (!ended.empty()) {                                // (4)
            if (i + 1 == n) fin.insert(fin.end(), ended.begin(), ended.end());
            else {
                bool possible = false;
                for (const Ref &x : ended) possible = possible || !e_->is_triv(x.id()) || (e_->triv_val(x.id()) & 1);
                if (possible) fin.push_back(regex_step({nz.zero(i + 1)}, ended));
            }
        }
        prev.swap(cur);
    }
    Ref r = or_tree(fin);
    if (e_->sum_c2(r.id()) > 1) r = pbs(r, LUT_NZ);          // a lone class flag or 1 - nz: a linear form
    return ch_flag(e_, r);
}

// ---------------------------------------------------------------------------------------------
// Where a match starts: re.match(pat, text, i) for every i at once, and re.search(pat, text).start()
// as the index of the first one.  The automaton runs BACKWARDS: `rev` = regex_reverse(pattern), read from the right,
//     back[q][i] = in_q(s[i]) & (q in rev.first  |  OR_{p in rev.pred(q)} back[p][i+1])         back[.][n] = 0
//     inside[i]  = no NUL among s[0 .. i-1]
//     start[i]   = inside[i] & OR_{q in rev.last} back[q][i]                  (nullable: start[i] = inside[i])
// rev.first are the pattern's last positions and rev.pred its follow sets, so back[q][i] says: from index i on, the
// characters can be read from position q to the end of a match.  No atom matches NUL, so a match that starts inside the
// text ends inside it: there is no end condition.  One pass, as deep as the string is long.
// ---------------------------------------------------------------------------------------------
int Strings::regex_find_trivial(const RegexProgram &rev, size_t n) {
    if (rev.nullable) return 1;
    return rev.min_len > n || n == 0 ? 0 : -1;
}

FStr Strings::regex_starts(const FStr &s, const RegexProgram &rev, const RegexPlan &plan) {
    if (regex_find_trivial(rev, s.size()) == 0) return FStr(s.size(), t(0));
    if (!fused()) return regex_starts_as_written(s, rev);
    FStr r;
    for (Ref f : f_regex_starts(s, rev, plan)) {
        if (e_->sum_c2(f.id()) > 1) f = pbs(f, LUT_NZ);      // a lone class flag: a linear form
        r.push_back(ch_flag(e_, f));
    }
    return r;
}

Pos Strings::regex_find(const FStr &s, const RegexProgram &rev, const RegexPlan &plan, size_t halves) {
    if (s.size() > ((size_t)1 << (8 * halves))) {             // as find_class: every index has to fit
        err = {FHS_ERR_LIMIT, LIMIT_MSG};
        return pos_trivial(0, halves);
    }
    const int k = regex_find_trivial(rev, s.size());
    if (k >= 0) return pos_trivial(k ? 0 : absent_value(halves), halves);
    if (fused()) return num_pos(f_find_digits(f_regex_starts(s, rev, plan), 4 * halves));
    Pos pos = pos_trivial(absent_value(halves), halves);
    const FStr flags = regex_starts_as_written(s, rev);
    for (size_t i = s.size(); i-- > 0;) pos_set_if(pos, flags[i], i);
    return pos;
}

// As written: the three formulas from char operations, in regex_as_written's style and with its algebra, which keeps what
// cannot end a match in the characters that are left free of charge; inside is a running bitand of ne(s[i], 0).
FStr Strings::regex_starts_as_written(const FStr &s, const RegexProgram &rev) {
    const size_t n = s.size(), P = rev.positions();
    const FChar zero = t(0), one = t(1);
    std::vector<FStr> tests(rev.classes.size(), FStr(n));    // [class][index]
    auto test = [&](size_t k, size_t i) {
        if (!tests[k][i].b[0]) tests[k][i] = class_test_as_written(s[i], rev.classes[k]);
        return tests[k][i];
    };
    FStr matches(n, one);                                    // OR_{q in rev.last} back[q][i]; a nullable pattern: 1
    std::vector<FChar> next(P, zero), cur(P, zero);
    for (size_t i = n; i-- > 0 && !rev.nullable;) {
        for (size_t q = 0; q < P; q++) {
            const FChar after = ((rev.first >> q) & 1) ? one : any_of(next, rev.pred[q]);
            cur[q] = flag_const(after) == 0 ? zero : flag_and(test((size_t)rev.cls[q], i), after);
        }
        matches[i] = any_of(cur, rev.last);
        next.swap(cur);
    }
    FStr r(n);
    FChar inside = one;
    for (size_t i = 0; i < n; i++) {
        if (i) inside = flag_and(inside, ch_ne(s[i - 1], zero));
        r[i] = flag_and(inside, matches[i]);
    }
    return r;
}

// Fused, on f_regex's parts.  (1) The class tests stand at the front (regex_class_tests).  (2) One regex_step per live
// (q, i), from the right: `in` the class flag(s), `preds` the back flags of rev.pred(q) at i + 1, or the trivial 1 for a
// q in rev.first, which folds the step to the AND of its class flags.  (3) (q, i) is live iff some position of rev.last
// (where a match starts) is at most i characters before q and some position of rev.first (where it ends) at most
// n - 1 - i characters after it, dead classes on neither way.  (4) start[i] is one more regex_step: in = inside[i] = 1 -
// Z[i], Z the exclusive prefix OR of the zero flags 1 - nz -- it stands beside the recurrence, log_15 n levels deep --
// preds = the back flags of rev.last at i: what acceptance does with end[j] in f_regex, so the text gate costs no level.
// The flags come back as they are (a class flag that no step refreshed may be a sum): regex_starts refreshes those,
// regex_find hands them to f_find_digits as find_class does.
std::vector<Ref> Strings::f_regex_starts(const FStr &s, const RegexProgram &rev, const RegexPlan &plan) {
    const size_t n = s.size(), P = rev.positions();
    const Ref one = trivial_block(e_, 1), zero = trivial_block(e_, 0);
    // characters from q on to the end of a match (0: q ends one), and from the start of a match up to q (0: q starts one)
    const std::vector<size_t> to_end = regex_distances(rev, plan, rev.first, rev.pred),
                              from_start = regex_distances(rev, plan, rev.last, rev.follow);
    std::vector<uint64_t> live(n, 0);
    size_t gates = 0;                                        // start flags are made below this index
    for (size_t i = 0; i < n; i++) {
        for (size_t q = 0; q < P; q++)
            if (to_end[q] != FAR && from_start[q] != FAR && from_start[q] <= i && to_end[q] <= n - 1 - i)
                live[i] |= (uint64_t)1 << q;
        if (rev.nullable || (live[i] & rev.last)) gates = i + 1;
    }
    NzMemo nz(this, s);
    const std::vector<std::vector<std::vector<Ref>>> in = regex_class_tests(s, rev, plan, live, nz);
    // inside[i] = 1 - Z[i]: the zero flags of the characters before the last gate, one unused flag behind (exclusive)
    std::vector<Ref> Z;
    if (gates) {
        std::vector<Ref> zf(gates, zero);
        for (size_t i = 0; i + 1 < gates; i++) zf[i] = nz.zero(i);
        Z = prefix_or(zf);
    }
    std::vector<Ref> start(n, zero), next(P), cur(P);
    for (size_t i = n; i-- > 0 && !err.code;) {
        std::vector<Ref> begun;
        for (size_t q = 0; q < P; q++) {
            cur[q] = Ref();
            if (!((live[i] >> q) & 1)) continue;
            std::vector<Ref> preds;
            if ((rev.first >> q) & 1) preds.push_back(one);
            for (size_t p = 0; p < P; p++)
                if (((rev.pred[q] >> p) & 1) && next[p]) preds.push_back(next[p]);
            cur[q] = regex_step(in[rev.cls[q]][i], preds);
            if ((rev.last >> q) & 1) begun.push_back(cur[q]);
        }
        if (i < gates) {
            if (rev.nullable) begun.assign(1, one);
            start[i] = regex_step({flag_not(Z[i])}, begun);
        }
        next.swap(cur);
    }
    return start;
}

}  // namespace fhs
