// String layer: host-side mirror of the reference's MyServerKey methods
// (src/server_key/mod.rs, src/server_key/trim.rs, src/utils.rs:28-112) as DAG constructors.
#pragma once
#include <utility>
#include <vector>

#include "radix.h"
#include "regex.h"

namespace fhs {

using FStr = std::vector<FChar>;   // FheString.bytes (fhestring.rs:6-9); cst = trivial 32 (:24)
// A position or count: one half for the reference's u8, two halves (lo, hi) for a 16-bit value lo + 256 * hi
using Pos = std::vector<FChar>;

struct StrError {
    int code = 0;   // FHS_ERR_LIMIT for the reference's panic!()
    const char *msg = "";
};

class Strings {
  public:
    explicit Strings(Engine *e) : e_(e) {}
    StrError err;

    FStr clear(const char *s, size_t n) const;   // the `_clear` twins trivially encrypt the pattern
    FChar contains(const FStr &s, const FStr &needle);
    FChar starts_with(const FStr &s, const FStr &pat);
    FChar ends_with(const FStr &s, const FStr &needle);
    FChar is_empty(const FStr &s);
    // find / rfind / len / the number of set 0/1 flags as a position of `halves` halves: 1 is the reference's u8 (absent =
    // 255, strings below 255 + |pattern| characters: src/main.rs:20, mod.rs:742-744, :1025-1027, :1044), 2 the same loops
    // and quirks on 16 bits (absent = 65535, strings below 65535 + |pattern|).  Past the limit: err, FHS_ERR_LIMIT.
    static constexpr const char *LIMIT_MSG = "Maximum supported size for find reached";
    static bool limit_reached(size_t n, size_t m, size_t halves);   // n counts the NUL that rfind pushes
    Pos find(const FStr &s, const FStr &pat, size_t halves = 1);
    Pos rfind(const FStr &s, const FStr &pat, size_t halves = 1);
    Pos len(const FStr &s, size_t halves = 1);
    Pos count_flags(const FStr &flags, size_t halves);
    // consumers of an encrypted position p on the n characters of s as they are, NULs included:
    // char_at = s[p] if p < n else 0; substr[j] = s[p + j] if p + j < n else 0, j < count; take[j] = s[j] if j < p else 0
    // (n characters); split_at = (take(s, p), substr(s, p, n)).  No length limit; an absent position is past the end.
    FChar char_at(const FStr &s, const Pos &pos);
    FStr substr(const FStr &s, const Pos &pos, size_t count);
    FStr take(const FStr &s, const Pos &pos);
    void split_at(const FStr &s, const Pos &pos, FStr *head, FStr *tail);
    // SQL LIKE against a CLEAR pattern (the reference has none).  Tokens: ANY = '%', any run of buffer
    // characters, NULs included; ONE = '_', one character that is not NUL; otherwise a literal byte, under ignore_case
    // (ASCII letters of the pattern only) either case of it.  Anchored at index 0; ends at j == n or s[j] == NUL.
    struct LikeTok { enum Kind : uint8_t { LIT, ONE, ANY } kind; uint8_t c; };
    // pat[m] with an optional escape byte (-1: none) -> tokens; false on a NUL, a bad escape byte or a dangling escape
    static bool like_parse(const char *pat, size_t m, int escape, std::vector<LikeTok> *out);
    // what the token counts alone decide on n characters: 0 (more ONE / LIT tokens than characters), 1 (ANY tokens only),
    // -1 otherwise
    static int like_trivial(const std::vector<LikeTok> &pat, size_t n);
    FChar like(const FStr &s, const std::vector<LikeTok> &pat, bool ignore_case);
    // A clear 256-entry table or a 256-bit set applied to every character of a buffer, NULs included (DESIGN.md section
    // 21).  The plan is made first and touches no operand: fused, it factors every output digit into user tables of the
    // engine (luts.h) and registers them; false with err = FHS_ERR_LIMIT when the registry is full.
    struct DigitPlan {
        enum Kind : uint8_t { PASS, CONST, ONE_LO, ONE_HI, PICK, LINES } kind = PASS;
        bool delta = false;                  // the construction gives out - in (mod 32), not out
        int konst = 0;                       // CONST
        int lut = 0;                         // ONE_LO / ONE_HI: the table; PICK: the pick table
        int lut_hi = 0, lut_lo = 0;          // PICK: the class of the high / low nibble ...
        int mul_hi = 1, mul_lo = 1;          // ... and their weights in the pick's index
        bool by_columns = false;             // LINES: flags of the low nibble, lines over the high one
        std::vector<std::pair<int, int>> lines;   // LINES: (flag table, line table) per distinct non-zero line
        int cost() const { return kind == PICK ? 3 : (kind == ONE_LO || kind == ONE_HI ? 1 : (kind == LINES ? 3 * (int)lines.size() : 0)); }
    };
    struct TablePlan {
        uint8_t table[256];                  // map: the table; class: 0/1 membership
        bool is_class = false;
        DigitPlan digit[4];                  // fused; a class uses digit[0]
    };
    bool plan_map(const uint8_t table[256], TablePlan *out);
    bool plan_class(const uint8_t set32[32], TablePlan *out);
    FStr map_clear(const FStr &s, const TablePlan &plan);                 // out[i] = table[s[i]]
    FStr class_flags(const FStr &s, const TablePlan &plan);               // 0/1 flag chars: s[i] in the set
    // index of the first character in the set, absent as find's; at most 256 (65536) characters
    Pos find_class(const FStr &s, const TablePlan &plan, size_t halves = 1);
    // A regular expression against a CLEAR pattern (the reference has none): the position automaton
    // of regex.h evaluated on the characters.  No atom matches NUL; anchored at index 0; ends at j == n or s[j] == NUL, as
    // LIKE does.  regex_trivial: what the automaton alone decides on n characters -- 0 (the shortest match is longer), 1
    // (it matches every text, or n == 0 and it is nullable), -1 otherwise.  regex_plan is made first and touches no operand: fused, every class that is
    // neither one byte (or the two cases of one letter), nor every character, gets the user tables of plan_class, and the
    // threshold tables the steps can ask for are registered; as written nothing is registered.  false with err =
    // FHS_ERR_LIMIT when the registry is full.
    struct RegexPlan {
        enum Kind : uint8_t { DEAD, ANY, BYTE, TABLE };      // per distinct class; DEAD: the empty set (\0)
        std::vector<Kind> kind;
        std::vector<uint8_t> byte;                            // BYTE: the byte, the upper case of a letter pair
        std::vector<char> both_cases;                         // BYTE: the byte | 0x20 is in the class as well
        std::vector<TablePlan> table;                         // TABLE (fused)
    };
    static int regex_trivial(const RegexProgram &g, size_t n);
    bool regex_plan(const RegexProgram &g, RegexPlan *out);
    FChar regex(const FStr &s, const RegexProgram &g, const RegexPlan &plan);
    // Where a match of a CLEAR pattern starts.  `rev` is regex_reverse of the pattern compiled
    // without search, `plan` is regex_plan(rev).  regex_starts: n 0/1 flag chars, out[i] = a match begins at i and no NUL
    // stands before i.  regex_find: the index of the first set flag as find_class returns it (absent: 255 / 65535; at
    // most 256 / 65536 characters).  regex_find_trivial: what the pattern alone decides on n characters -- 1: nullable,
    // find is 0 (starts still depends on the string); 0: not nullable and min_len > n or n == 0, find is absent and every
    // start flag 0; -1 otherwise.
    static int regex_find_trivial(const RegexProgram &rev, size_t n);
    FStr regex_starts(const FStr &s, const RegexProgram &rev, const RegexPlan &plan);
    Pos regex_find(const FStr &s, const RegexProgram &rev, const RegexPlan &plan, size_t halves = 1);
    FChar eq(const FStr &a, const FStr &b);
    FChar ne(const FStr &a, const FStr &b);
    FChar eq_ignore_case(const FStr &a, const FStr &b);
    FChar comparison(const FStr &a, const FStr &b, int cmp);   // 0 lt, 1 le, 2 gt, 3 ge
    // positional half on two equally long slices: (any position differs, verdict at the first differing position)
    void f_cmp_partial(const FStr &a, const FStr &b, int cmp, FChar *any_diff_out, FChar *verdict_out);
    // combine such partials over consecutive ranges: the first range that differs decides, `tie` if none does
    FChar flags_first_decides(const FStr &any_diff, const FStr &verdict, int tie);
    // window-sharded find (multi-GPU): the match flags of a slice's windows, and the rest of find on ALL flags in string
    // order (index of the first one set, 255 if none; at most 256 flags, which the limit on the whole string guarantees)
    // -- fhs_dist_str_find exchanges the flags in between
    std::vector<Ref> f_find_window_flags(const FStr &s, const FStr &pat);
    FChar f_find_from_flags(const std::vector<Ref> &flags);
    FStr to_upper(const FStr &s);
    FStr to_lower(const FStr &s);
    FStr replace(const FStr &s, const FStr &from, const FStr &to);
    FStr replacen(const FStr &s, const FStr &from, const FStr &to, const FChar &n);
    FStr repeat(const FStr &s, const FChar &n);
    FStr repeat_clear(const FStr &s, size_t n);
    FStr concatenate(const FStr &a, const FStr &b);
    FStr strip_prefix(const FStr &s, const FStr &pat, FChar *found);
    FStr strip_suffix(const FStr &s, const FStr &pat, FChar *found);
    FStr trim_end(const FStr &s);
    FStr trim_start(const FStr &s);
    FStr trim(const FStr &s);
    FStr bubble_zeroes_right(const FStr &s);
    FChar flags_or(const FStr &flags);
    FChar flags_and(const FStr &flags);
    // split family (src/server_key/split.rs): result[buffer][position] + pattern_found, like FheSplit
    enum SplitKind { SPLIT = 0, SPLIT_INCLUSIVE, SPLIT_TERMINATOR, SPLITN, RSPLIT, RSPLIT_TERMINATOR, RSPLITN,
                     RSPLIT_ONCE, SPLIT_ASCII_WHITESPACE };
    std::vector<FStr> split_family(int kind, const FStr &s, const FStr &pat, const FChar *n, FChar *found);

  private:
    Engine *e_;
    bool fused() const { return e_->mode == 1; }
    FChar t(uint8_t v) const { return ch_trivial(e_, v); }
    typedef std::vector<Ref> Num;   // little-endian base-4 digits, clean (<= 3)

    // ---- single-block 0/1 flags (fused mode) ----
    Ref flag_not(const Ref &x);                                       // 1 - x, a linear form
    bool drop_trivial(std::vector<Ref> &flags, int absorbing) const;  // false: a trivial flag decides, the result is `absorbing`
    Ref flag_tree(std::vector<Ref> flags, int absorbing);             // log_15-depth AND (absorbing = 0) or OR (1)
    Ref and_tree(std::vector<Ref> flags) { return flag_tree(std::move(flags), 0); }
    Ref or_tree(std::vector<Ref> flags) { return flag_tree(std::move(flags), 1); }
    Ref onehot_or(std::vector<Ref> flags);   // OR of flags of which at most one is set: noise-budget-wide groups
    std::vector<Ref> prefix_or(const std::vector<Ref> &f);            // exclusive: OR_{k<i}
    std::vector<Ref> suffix_or(const std::vector<Ref> &f);            // exclusive: OR_{k>i}
    Ref lin_in_budget(Ref *const blk[4], const int64_t coef[4]);      // sum coef * blk, the sums among blk refreshed if it must
    std::vector<Ref> block_eq_flags(const FChar &a, const FChar &b);
    std::vector<Ref> byte_eq_flags(const FChar &c, uint8_t byte, bool both_cases);   // the nibble flags of c == byte (either case)
    Ref window_match(const FStr &s, size_t at, const FStr &pat);
    Ref char_zero_test(const FChar &c, bool want_zero);               // 1 block, 1 bootstrap: c == 0 / c != 0
    struct NzMemo {                                                   // nz(i) = [s[i] != 0], made on first use and shared
        Strings *str;
        const FStr &s;
        std::vector<Ref> made;
        NzMemo(Strings *str_, const FStr &s_) : str(str_), s(s_), made(s_.size()) {}
        Ref operator()(size_t i) {
            if (!made[i]) made[i] = str->char_zero_test(s[i], false);
            return made[i];
        }
        Ref zero(size_t i) { return str->flag_not((*this)(i)); }      // [s[i] == 0] = 1 - nz(i)
    };
    Ref char_significant(const FChar &c);                             // 1 block: c is neither NUL nor whitespace
    Ref is_upper_flag(const FChar &c, bool lower);
    FChar ite_flag(const Ref &flag, const FChar &t, const FChar &f);

    // ---- positions and counts: find, rfind, len, count_flags ----
    Pos pos_trivial(unsigned v, size_t halves) const;
    static FChar num_char(const Num &v, size_t first_digit = 0);      // four digits of a number as a char
    static Pos num_pos(const Num &v);                                 // four digits to a half
    // as written: the position update, the counter and the window test of the reference's loops
    void pos_set_if(Pos &pos, const FChar &flag, size_t v);
    void pos_add_flag(Pos &counter, const FChar &flag);
    FChar window_eq(const FStr &s, size_t at, const FStr &pat, bool downwards);
    Pos count(const FStr &s, bool are_flags, size_t halves);
    // fused: flags first, then the digits of the result (4 to a half)
    Num f_find_digits(const std::vector<Ref> &flags, size_t digits);
    Num f_rfind_digits(const FStr &s, const FStr &pat, size_t digits);
    Num first_index(const std::vector<Ref> &before, const Ref &found, size_t digits);
    Num position_of(const std::vector<Ref> &pick, size_t index_offset, const Ref *absent_flag, int absent_value, size_t digits);
    Num count_flags(const std::vector<Ref> &flags, size_t digits);   // sum of 0/1 flags mod 4^digits

    // ---- positions as operands: one implementation over the halves of the position ----
    FChar pos_eq(const Pos &pos, size_t i);                            // as written: pos == i
    FChar pos_gt(const Pos &pos, size_t j);                            // as written: pos > j
    Num pos_digits(const Pos &pos);                                    // 4 or 8 digits, each at sum c^2 <= 4
    struct PosBits { int K = 0; std::vector<Ref> bit; Ref ovf; };      // bits 0 .. K-1 as 0/1 blocks, ovf = some bit >= K is set
    PosBits f_pos_bits(const Num &dg, size_t n);
    FStr f_pos_shift(const FStr &s, const Num &dg, size_t count);      // out[j] = s[p + j]
    std::vector<Ref> f_pos_thermometer(const Num &dg, size_t limit);   // g[j] = [p > j], j < limit <= 4^digits
    FStr f_pos_take(const FStr &s, const Num &dg);

    // ---- fused forms of the tests, comparisons and maps ----
    FChar f_contains(const FStr &s, const FStr &needle);
    FChar f_ends_with(const FStr &s, const FStr &needle, std::vector<Ref> *pick_out);
    // as written: 0/1 flag chars with trivial constants folded away (LIKE, regex)
    int flag_const(const FChar &f) const;
    FChar flag_and(const FChar &a, const FChar &b);
    FChar flag_or(const FChar &a, const FChar &b);
    FChar any_of(const std::vector<FChar> &flags, uint64_t set);
    FChar class_test_as_written(const FChar &c, const RegexClass &cls);
    FChar like_as_written(const FStr &s, const std::vector<LikeTok> &pat, bool ignore_case);
    FChar f_like(const FStr &s, const std::vector<LikeTok> &pat, bool ignore_case);
    FChar regex_as_written(const FStr &s, const RegexProgram &g);
    FChar f_regex(const FStr &s, const RegexProgram &g, const RegexPlan &plan);
    Ref regex_step(std::vector<Ref> in, std::vector<Ref> preds);      // AND of the flags `in` AND (OR of `preds`)
    // fused class tests of f_regex / f_regex_starts: [class][index] -> one flag, or the two nibble flags of a BYTE class,
    // where live[index] holds a position of that class
    std::vector<std::vector<std::vector<Ref>>> regex_class_tests(const FStr &s, const RegexProgram &g, const RegexPlan &plan,
                                                                 const std::vector<uint64_t> &live, NzMemo &nz);
    FStr regex_starts_as_written(const FStr &s, const RegexProgram &rev);
    std::vector<Ref> f_regex_starts(const FStr &s, const RegexProgram &rev, const RegexPlan &plan);
    FChar f_eq(const FStr &a, const FStr &b);
    FChar f_eq_ignore_case(const FStr &a, const FStr &b);
    // lexicographic order as a tree of three-state values s = sign(a - b) in {-1, 0, 1}, most significant first
    std::vector<Ref> cmp_leaves(const FStr &a, const FStr &b);          // one per nibble pair, missing characters are 0
    Ref cmp_root_sum(std::vector<Ref> states);                          // 8 + 4 s1 + 2 s2 + s3 of the last <= 3 states
    FChar f_comparison(const FStr &a, const FStr &b, int cmp);
    FStr f_case(const FStr &s, bool to_lower);
    FStr f_trim(const FStr &s, bool from_end);

    // ---- clear tables and sets ----
    bool plan_matrix(const uint8_t m[16][16], bool allow_lines, bool dry, DigitPlan *out);
    int user_table(const uint8_t values[16]);                          // registers; -1 and err when the registry is full
    void nibbles(FChar &c, Ref *lo, Ref *hi);                          // b0 + 4 b1, b2 + 4 b3; refreshes c where it must
    Ref apply_digit(const DigitPlan &p, const Ref &lo, const Ref &hi);
    std::vector<Ref> f_class_flags(const FStr &s, const TablePlan &plan);

    // ---- replace ----
    FStr longer_from(const FStr &s, const FStr &from, FStr to, const FChar &n, bool use_counter);
    FStr shorter_from(const FStr &s, const FStr &from, const FStr &to, const FChar &n, bool use_counter);
    FStr f_replace_expand(const FStr &s, const FStr &from, const FStr &to);

    // ---- oblivious compaction: replaces the O(n^2) bubble of utils.rs:28-46 in fused mode ----
    std::vector<Num> flag_prefix_counts(const std::vector<Ref> &flags, size_t digits);   // exclusive
    Num num_add(const std::vector<const Num *> &ops, size_t digits);
    Num count_digits(const Ref *flags, size_t k, size_t digits);   // sum of <= 15 flags as a base-4 number, within the noise budget
    std::vector<Num> num_exclusive_scan(const std::vector<Num> &x, size_t digits);
    FStr f_compact(const FStr &s);

    // ---- split family: char-level ops as written, or single-block-flag versions in fused mode ----
    FChar s_eq(const FChar &a, const FChar &b);
    FChar s_ite(const FChar &flag, const FChar &tv, const FChar &fv);
    FChar s_not(const FChar &flag);
    FChar split_match(bool reverse, size_t i, const FStr &s, const FStr &pat, FStr &mask);
    std::vector<FStr> xsplit(const FStr &s, const FStr &pat, bool inclusive, bool terminator, const FChar *n,
                             bool reverse, FChar *found);
    // fused formulation of the distribution phase (buffer ids as prefix counts, multi-digit, membership selects)
    bool f_split_distribute(const FStr &s, const FStr &pat, const FChar *n, bool reverse, std::vector<FStr> &result,
                            FChar *found);
    void split_cleanup(std::vector<FStr> &result, const FStr &pat, bool inclusive, bool terminator, const FChar *n);
    FStr on_support(const FStr &row, FStr (Strings::*op)(const FStr &, const FStr &, const FStr &), const FStr &a,
                    const FStr &b);
    std::vector<FStr> split_ws(const FStr &s, FChar *found);
};

}  // namespace fhs
