// String layer, part 6 of 7: clear tables and classes (map_clear, class_flags, find_class).
#include "strings.h"

#include <algorithm>
#include <cstring>
#include <set>

#include "strings_internal.h"

namespace fhs {

// ---------------------------------------------------------------------------------------------
// clear tables and sets on encrypted characters: map_clear, class_flags, find_class.  The
// reference has five hand-built instances (to_upper, to_lower, is_whitespace, is_uppercase, is_lowercase); here the
// table is the caller's.  A character is taken as it is, NUL included.
// ---------------------------------------------------------------------------------------------
int Strings::user_table(const uint8_t values[16]) {
    const int id = user_lut_register(values);
    if (id < 0) err = {FHS_ERR_LIMIT, "the registry of user look-up tables is full"};
    return id;
}

// One output digit as a 16 x 16 matrix m[hi][lo] of block values.  With R distinct rows and C distinct columns:
// R = C = 1 a constant; R = 1 (C = 1) one table on the low (high) nibble; R C <= 16 the class of the row, the class of
// the column and a pick table on the index they form, the smaller of R and C as the multiplier (<= 4: sum c^2 <= 17);
// otherwise, where the values are plain digits (allow_lines), per distinct non-zero row a flag of the high nibble, the
// row as a table of the low one and LUT_SEL_T on 4 flag + row -- or the same by columns if those are fewer.
// dry: the shape and its cost only, nothing is registered.
bool Strings::plan_matrix(const uint8_t m[16][16], bool allow_lines, bool dry, DigitPlan *out) {
    auto table = [&](const uint8_t values[16]) { return dry ? 0 : user_table(values); };
    int row_cls[16], col_cls[16], row_rep[16], col_rep[16], R = 0, C = 0;
    for (int h = 0; h < 16; h++) {
        int k = 0;
        while (k < R && std::memcmp(m[row_rep[k]], m[h], 16) != 0) k++;
        if (k == R) row_rep[R++] = h;
        row_cls[h] = k;
    }
    for (int l = 0; l < 16; l++) {
        int k = 0;
        auto same = [&](int a, int b) {
            for (int h = 0; h < 16; h++)
                if (m[h][a] != m[h][b]) return false;
            return true;
        };
        while (k < C && !same(col_rep[k], l)) k++;
        if (k == C) col_rep[C++] = l;
        col_cls[l] = k;
    }
    DigitPlan p;
    uint8_t v[16] = {0}, w[16] = {0};
    if (R == 1 && C == 1) {
        p.kind = DigitPlan::CONST;
        p.konst = m[0][0];
    } else if (R == 1 || C == 1) {
        p.kind = R == 1 ? DigitPlan::ONE_LO : DigitPlan::ONE_HI;
        for (int x = 0; x < 16; x++) v[x] = R == 1 ? m[0][x] : m[x][0];
        if ((p.lut = table(v)) < 0) return false;
    } else if (R * C <= 16) {
        p.kind = DigitPlan::PICK;
        p.mul_hi = R <= C ? 1 : C;
        p.mul_lo = R <= C ? R : 1;
        for (int x = 0; x < 16; x++) { v[x] = (uint8_t)row_cls[x]; w[x] = (uint8_t)col_cls[x]; }
        if ((p.lut_hi = table(v)) < 0 || (p.lut_lo = table(w)) < 0) return false;
        uint8_t pick[16] = {0};
        for (int r = 0; r < R; r++)
            for (int c = 0; c < C; c++) pick[p.mul_hi * r + p.mul_lo * c] = m[row_rep[r]][col_rep[c]];
        if ((p.lut = table(pick)) < 0) return false;
    } else {
        if (!allow_lines) return false;
        auto zero_row = [&](int h) { for (int l = 0; l < 16; l++) if (m[h][l]) return false; return true; };
        auto zero_col = [&](int l) { for (int h = 0; h < 16; h++) if (m[h][l]) return false; return true; };
        int nr = 0, nc = 0;
        for (int k = 0; k < R; k++) nr += !zero_row(row_rep[k]);
        for (int k = 0; k < C; k++) nc += !zero_col(col_rep[k]);
        p.kind = DigitPlan::LINES;
        p.by_columns = nc < nr;
        const int n = p.by_columns ? C : R;
        for (int k = 0; k < n; k++) {
            const int rep = p.by_columns ? col_rep[k] : row_rep[k];
            if (p.by_columns ? zero_col(rep) : zero_row(rep)) continue;
            for (int x = 0; x < 16; x++) {
                v[x] = (p.by_columns ? col_cls[x] : row_cls[x]) == k;
                w[x] = p.by_columns ? m[x][rep] : m[rep][x];
            }
            const int flag = table(v), line = table(w);
            if (flag < 0 || line < 0) return false;
            p.lines.push_back({flag, line});
        }
    }
    *out = p;
    return true;
}

// Per output digit d the matrix of out_d - in_d (mod 32): out_d = in_d + that is exact and lies in [0, 4); where it is
// zero the block passes through.  The matrix of out_d itself is tried as well and taken where it is no dearer (its
// result is one bootstrap output, not a sum with the operand's block); neither being a constant, one table or a pick,
// out_d is built line by line.
bool Strings::plan_map(const uint8_t table[256], TablePlan *out) {
    std::memcpy(out->table, table, 256);
    out->is_class = false;
    if (!fused()) return true;
    for (int d = 0; d < 4; d++) {
        uint8_t plain[16][16], delta[16][16];
        bool same = true;
        for (int x = 0; x < 256; x++) {
            const int in = (x >> (2 * d)) & 3, o = (table[x] >> (2 * d)) & 3;
            plain[x >> 4][x & 15] = (uint8_t)o;
            delta[x >> 4][x & 15] = (uint8_t)((o - in) & 31);
            same = same && o == in;
        }
        DigitPlan &p = out->digit[d];
        p = DigitPlan();
        if (same) continue;
        DigitPlan a, b;
        const bool has_b = plan_matrix(delta, false, true, &b);
        plan_matrix(plain, true, true, &a);
        const bool use_delta = has_b && b.cost() < a.cost();  // (a constant shift of the digit costs no bootstrap)
        if (!plan_matrix(use_delta ? delta : plain, !use_delta, false, &p)) return false;
        p.delta = use_delta;
    }
    return true;
}

bool Strings::plan_class(const uint8_t set32[32], TablePlan *out) {
    uint8_t m[16][16];
    for (int x = 0; x < 256; x++) out->table[x] = m[x >> 4][x & 15] = (set32[x >> 3] >> (x & 7)) & 1;
    out->is_class = true;
    if (!fused()) return true;
    return plan_matrix(m, true, false, &out->digit[0]);
}

// The nibbles of a character as bootstrap inputs.  Blocks that are sums of bootstrap outputs are refreshed where the
// weights 1, 4 would leave the noise budget (LUT_MSG keeps a clean digit), as block_eq_flags does; c keeps the refreshed
// blocks, so what passes through to the result is the refreshed block too.
void Strings::nibbles(FChar &c, Ref *lo, Ref *hi) {
    for (int h = 0; h < 2; h++) {
        Ref &a = c.b[2 * h], &b = c.b[2 * h + 1];
        Ref d = lin(e_, {{1, &a}, {4, &b}});
        if (e_->sum_c2(d.id()) > FHS_NOISE_BUDGET_SUM_C2) {
            if (e_->sum_c2(a.id()) > 1) a = pbs(a, LUT_MSG);
            if (e_->sum_c2(b.id()) > 1) b = pbs(b, LUT_MSG);
            d = lin(e_, {{1, &a}, {4, &b}});
        }
        *(h ? hi : lo) = d;
    }
}

Ref Strings::apply_digit(const DigitPlan &p, const Ref &lo, const Ref &hi) {
    switch (p.kind) {
        case DigitPlan::CONST: return trivial_block(e_, p.konst);
        case DigitPlan::ONE_LO: return pbs(lo, p.lut);
        case DigitPlan::ONE_HI: return pbs(hi, p.lut);
        case DigitPlan::PICK: {
            Ref k = pbs(hi, p.lut_hi), l = pbs(lo, p.lut_lo);
            return pbs(lin(e_, {{p.mul_hi, &k}, {p.mul_lo, &l}}), p.lut);
        }
        case DigitPlan::LINES: {
            // at most one selection is non-zero, so every partial sum is a digit; more than four are refreshed
            std::vector<Ref> sel;
            for (const auto &fl : p.lines) {
                Ref f = pbs(p.by_columns ? lo : hi, fl.first), r = pbs(p.by_columns ? hi : lo, fl.second);
                sel.push_back(pbs(lin(e_, {{4, &f}, {1, &r}}), LUT_SEL_T));
            }
            Ref sum = sum_refs(e_, sel.data(), sel.size());
            return sel.size() > 4 ? pbs(sum, LUT_MSG) : sum;
        }
        default: break;
    }
    return trivial_block(e_, 0);
}

FStr Strings::map_clear(const FStr &s, const TablePlan &plan) {
    FStr r;
    r.reserve(s.size());
    if (!fused()) {
        // as written: out = c; for every v with table[v] != v, ascending: out = if_then_else(c == v, table[v], out)
        for (const FChar &c : s) {
            FChar o = c;
            for (int v = 0; v < 256; v++)
                if (plan.table[v] != v) o = ch_ite(ch_eq(c, t((uint8_t)v)), t(plan.table[v]), o);
            r.push_back(o);
        }
        return r;
    }
    bool any = false;
    for (int d = 0; d < 4; d++) any = any || plan.digit[d].kind != DigitPlan::PASS;
    for (const FChar &c_in : s) {
        FChar c = c_in, o;
        Ref lo, hi;
        if (any) nibbles(c, &lo, &hi);
        for (int d = 0; d < 4; d++) {
            const DigitPlan &p = plan.digit[d];
            if (p.kind == DigitPlan::PASS) { o.b[d] = c.b[d]; continue; }
            Ref x = apply_digit(p, lo, hi);
            o.b[d] = p.delta ? lin(e_, {{1, &c.b[d]}, {1, &x}}) : x;
        }
        r.push_back(o);
    }
    return r;
}

std::vector<Ref> Strings::f_class_flags(const FStr &s, const TablePlan &plan) {
    const DigitPlan &p = plan.digit[0];
    std::vector<Ref> f;
    f.reserve(s.size());
    for (const FChar &c_in : s) {
        if (p.kind == DigitPlan::CONST) { f.push_back(trivial_block(e_, p.konst)); continue; }
        FChar c = c_in;
        Ref lo, hi;
        nibbles(c, &lo, &hi);
        if (p.kind != DigitPlan::LINES) { f.push_back(apply_digit(p, lo, hi)); continue; }
        std::vector<Ref> sel;                                 // one-hot: handed back at sum c^2 <= 4 (onehot_or)
        for (const auto &fl : p.lines) {
            Ref e = pbs(p.by_columns ? lo : hi, fl.first), r = pbs(p.by_columns ? hi : lo, fl.second);
            sel.push_back(pbs(lin(e_, {{4, &e}, {1, &r}}), LUT_SEL_T));
        }
        f.push_back(onehot_or(sel));
    }
    return f;
}

FStr Strings::class_flags(const FStr &s, const TablePlan &plan) {
    FStr r;
    r.reserve(s.size());
    if (fused()) {
        for (const Ref &f : f_class_flags(s, plan)) r.push_back(ch_flag(e_, f));
        return r;
    }
    for (const FChar &c : s) {                                // as written: the OR of c == v over the members
        FChar f = t(0);
        for (int v = 0; v < 256; v++)
            if (plan.table[v]) f = ch_bitor(f, ch_eq(c, t((uint8_t)v)));
        r.push_back(f);
    }
    return r;
}

Pos Strings::find_class(const FStr &s, const TablePlan &plan, size_t halves) {
    if (s.size() > ((size_t)1 << (8 * halves))) {             // every index has to fit; the last one reads as absent
        err = {FHS_ERR_LIMIT, LIMIT_MSG};
        return pos_trivial(0, halves);
    }
    Pos pos = pos_trivial(absent_value(halves), halves);
    if (s.empty()) return pos;
    if (fused()) return num_pos(f_find_digits(f_class_flags(s, plan), 4 * halves));
    const FStr flags = class_flags(s, plan);
    for (size_t i = s.size(); i-- > 0;) pos_set_if(pos, flags[i], i);
    return pos;
}

}  // namespace fhs
