// Parser and position automaton of regex_clear.  The syntax is a strict subset of Python's bytes
// `re`: whatever is accepted here means there what it means here, and everything else is refused with the offset of its
// first byte.
#include "regex.h"

#include <algorithm>
#include <cstring>

namespace fhs {

int RegexClass::count() const {
    int n = 0;
    for (int v = 0; v < 256; v++) n += has(v);
    return n;
}
bool RegexClass::operator==(const RegexClass &o) const { return std::memcmp(bits, o.bits, 32) == 0; }

bool RegexProgram::matches_everything() const {
    if (!nullable) return false;
    for (size_t q = 0; q < positions(); q++) {
        const uint64_t bit = (uint64_t)1 << q;
        if (classes[cls[q]].count() == 255 && (first & bit) && (follow[q] & bit) && (last & bit)) return true;
    }
    return false;
}

namespace {

constexpr uint32_t INF = 0xFFFFFFFFu;
constexpr uint32_t REPEAT_CAP = 1u << 20;      // larger counts saturate: they are past the position limit anyway
constexpr int MAX_DEPTH = 64;                  // nested groups
constexpr size_t MAX_ATOMS = 1024;             // written atoms, groups and '|' together (the tree is walked recursively)

bool is_letter(int c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }
bool is_digit(int c) { return c >= '0' && c <= '9'; }
bool is_alnum(int c) { return is_letter(c) || is_digit(c); }
int hex_value(int c) {
    if (is_digit(c)) return c - '0';
    if (c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

struct Node {
    enum Kind : uint8_t { EMPTY, CLASS, CAT, ALT, REPEAT } kind = EMPTY;
    int a = -1, b = -1;
    uint32_t min = 0, max = 0;                 // REPEAT; max == INF: unbounded
    RegexClass set;                            // CLASS
};

struct Frag {                                  // a compiled sub-expression
    bool nullable = true;
    uint64_t first = 0, last = 0;
};

class Compiler {
  public:
    Compiler(const char *pat, size_t m, bool ignore_case) : p_((const uint8_t *)pat), m_(m), ic_(ignore_case) {}
    RegexStatus status = REGEX_OK;
    size_t err_offset = 0;
    const char *err_msg = "";

    int parse() {
        const int root = alt(0);
        if (status == REGEX_OK && at_ < m_) fail(at_, "unbalanced ')'");   // alt() stops at a ')' it has no '(' for
        return root;
    }
    int wrap_search(int root) {                // .*(?:root).*
        RegexClass any = shorthand('.');
        auto star_any = [&] { return repeat(leaf(any), 0, INF); };
        const int head = star_any(), tail = star_any();   // (two calls, two nodes, in this order)
        return cat(cat(head, root), tail);
    }
    uint64_t count(int n) const {              // positions after expansion, saturating
        const Node &x = nodes_[n];
        switch (x.kind) {
            case Node::CLASS: return 1;
            case Node::CAT: case Node::ALT: return std::min<uint64_t>(count(x.a) + count(x.b), (uint64_t)1 << 40);
            case Node::REPEAT: {
                const uint64_t copies = x.max == INF ? std::max<uint32_t>(x.min, 1) : x.max;
                return std::min<uint64_t>(count(x.a) * copies, (uint64_t)1 << 40);
            }
            default: return 0;
        }
    }
    uint64_t min_len(int n) const {
        const Node &x = nodes_[n];
        switch (x.kind) {
            case Node::CLASS: return 1;
            case Node::CAT: return std::min<uint64_t>(min_len(x.a) + min_len(x.b), (uint64_t)1 << 40);
            case Node::ALT: return std::min(min_len(x.a), min_len(x.b));
            case Node::REPEAT: return std::min<uint64_t>(min_len(x.a) * x.min, (uint64_t)1 << 40);
            default: return 0;
        }
    }
    // Glushkov: every call allots fresh positions, so a counted repeat builds its operand once per copy
    Frag build(int n, RegexProgram *g) const {
        const Node &x = nodes_[n];
        switch (x.kind) {
            case Node::CLASS: {
                const size_t q = g->cls.size();
                size_t k = 0;
                while (k < g->classes.size() && !(g->classes[k] == x.set)) k++;
                if (k == g->classes.size()) g->classes.push_back(x.set);
                g->cls.push_back((int)k);
                g->follow.push_back(0);
                Frag f;
                f.nullable = false;
                f.first = f.last = (uint64_t)1 << q;
                return f;
            }
            case Node::CAT: {
                const Frag a = build(x.a, g);          // (sequenced: positions number from left to right)
                const Frag b = build(x.b, g);
                return cat_frag(a, b, g);
            }
            case Node::ALT: {
                const Frag a = build(x.a, g);
                const Frag b = build(x.b, g);
                Frag f;
                f.nullable = a.nullable || b.nullable;
                f.first = a.first | b.first;
                f.last = a.last | b.last;
                return f;
            }
            case Node::REPEAT: {
                Frag f;
                if (count(x.a) == 0) return f;         // an operand without positions matches the empty string only
                const uint32_t plain = x.max == INF ? (x.min ? x.min - 1 : 0) : x.min;
                for (uint32_t i = 0; i < plain; i++) f = cat_frag(f, build(x.a, g), g);
                if (x.max == INF) {                    // the last copy loops; with min == 0 it may be skipped as well
                    Frag r = build(x.a, g);
                    link(r.last, r.first, g);
                    if (x.min == 0) r.nullable = true;
                    f = cat_frag(f, r, g);
                } else {
                    for (uint32_t i = x.min; i < x.max; i++) {
                        Frag r = build(x.a, g);
                        r.nullable = true;
                        f = cat_frag(f, r, g);
                    }
                }
                return f;
            }
            default: return Frag();
        }
    }

  private:
    const uint8_t *p_;
    size_t m_, at_ = 0, atoms_ = 0;
    bool ic_;
    std::vector<Node> nodes_;

    int fail(size_t offset, const char *msg, RegexStatus st = REGEX_SYNTAX) {
        if (status == REGEX_OK) { status = st; err_offset = offset; err_msg = msg; }
        at_ = m_;
        return empty();
    }
    int empty() { nodes_.emplace_back(); return (int)nodes_.size() - 1; }
    int leaf(const RegexClass &set) {
        Node x;
        x.kind = Node::CLASS;
        x.set = set;
        x.set.bits[0] &= 0xFE;                 // no atom matches NUL
        nodes_.push_back(x);
        return (int)nodes_.size() - 1;
    }
    int pair(Node::Kind k, int a, int b) {
        Node x;
        x.kind = k;
        x.a = a;
        x.b = b;
        nodes_.push_back(x);
        return (int)nodes_.size() - 1;
    }
    int cat(int a, int b) {
        if (nodes_[a].kind == Node::EMPTY) return b;
        if (nodes_[b].kind == Node::EMPTY) return a;
        return pair(Node::CAT, a, b);
    }
    int repeat(int a, uint32_t lo, uint32_t hi) {
        Node x;
        x.kind = Node::REPEAT;
        x.a = a;
        x.min = lo;
        x.max = hi;
        nodes_.push_back(x);
        return (int)nodes_.size() - 1;
    }
    static void link(uint64_t from, uint64_t to, RegexProgram *g) {
        for (size_t q = 0; q < g->follow.size(); q++)
            if ((from >> q) & 1) g->follow[q] |= to;
    }
    static Frag cat_frag(const Frag &a, const Frag &b, RegexProgram *g) {
        link(a.last, b.first, g);
        Frag f;
        f.nullable = a.nullable && b.nullable;
        f.first = a.first | (a.nullable ? b.first : 0);
        f.last = b.last | (b.nullable ? a.last : 0);
        return f;
    }

    // ---- sets ----
    static RegexClass shorthand(int c) {       // . d w s and the complements D W S (NUL is removed by leaf())
        RegexClass s;
        const int lower = c | 0x20;
        for (int v = 0; v < 256; v++) {
            const bool in = c == '.' ? true
                          : lower == 'd' ? is_digit(v)
                          : lower == 'w' ? (is_alnum(v) || v == '_')
                                         : (v == ' ' || (v >= '\t' && v <= '\r'));
            if (in != (c == 'D' || c == 'W' || c == 'S')) s.add(v);
        }
        return s;
    }
    void close_case(RegexClass *s) const {
        if (!ic_) return;
        for (int v = 'A'; v <= 'Z'; v++)
            if (s->has(v) || s->has(v | 0x20)) { s->add(v); s->add(v | 0x20); }
    }
    // what follows a backslash at at_ - 1: a byte (>= 0), a shorthand set (-2, in *set) or an error (-1)
    int escape(bool in_class, RegexClass *set) {
        const size_t start = at_ - 1;
        if (at_ >= m_) { fail(start, "a backslash at the end of the pattern"); return -1; }
        const int c = p_[at_++];
        switch (c) {
            case 0: fail(at_ - 1, "a NUL byte in the pattern"); return -1;
            case 't': return '\t';
            case 'n': return '\n';
            case 'r': return '\r';
            case 'f': return '\f';
            case 'v': return '\v';
            case '0':
                if (at_ < m_ && is_digit(p_[at_])) { fail(start, "octal escapes other than \\0 are not supported"); return -1; }
                return 0;
            case 'x': {
                const int h = at_ + 1 < m_ ? hex_value(p_[at_]) : -1, l = at_ + 1 < m_ ? hex_value(p_[at_ + 1]) : -1;
                if (h < 0 || l < 0) { fail(start, "\\x needs two hexadecimal digits"); return -1; }
                at_ += 2;
                return 16 * h + l;
            }
            case 'd': case 'w': case 's': case 'D': case 'W': case 'S':
                *set = shorthand(c);
                return -2;
            default: break;
        }
        if (is_alnum(c)) {
            fail(start, in_class ? "this escape is not supported in a class"
                                 : "anchors, word boundaries, back-references and other letter escapes are not supported");
            return -1;
        }
        return c;                              // a backslash in front of anything else: that byte
    }
    int char_class() {                         // at_ is behind the '['
        const size_t open = at_ - 1;
        bool negate = false;
        if (at_ < m_ && p_[at_] == '^') { negate = true; at_++; }
        if (at_ < m_ && p_[at_] == ']') return fail(open, "an empty class");
        RegexClass set;
        const size_t body = at_;
        for (;;) {
            if (at_ >= m_) return fail(open, "unbalanced '['");
            const size_t item = at_;
            int c = p_[at_++];
            if (c == ']') break;
            if (c == 0) return fail(item, "a NUL byte in the pattern");
            if (c == '[' && item == body) return fail(item, "an unescaped '[' at the start of a class");
            if ((c == '-' || c == '&' || c == '~' || c == '|') && at_ < m_ && p_[at_] == c)
                return fail(item, "a doubled set operator in a class");
            RegexClass sub;
            if (c == '\\' && (c = escape(true, &sub)) == -1) return empty();
            if (c == -2) {
                if (at_ + 1 < m_ && p_[at_] == '-' && p_[at_ + 1] != ']') return fail(item, "a range from a class shorthand");
                for (int k = 0; k < 32; k++) set.bits[k] |= sub.bits[k];
                continue;
            }
            int hi = c;
            if (at_ + 1 < m_ && p_[at_] == '-' && p_[at_ + 1] != ']') {   // a range; a '-' in front of the ']' is itself
                at_++;
                hi = p_[at_++];
                if (hi == 0) return fail(at_ - 1, "a NUL byte in the pattern");
                if (hi == '\\' && (hi = escape(true, &sub)) == -1) return empty();
                if (hi == -2) return fail(item, "a range up to a class shorthand");
                if (hi < c) return fail(item, "a reversed range");
            }
            for (int v = c; v <= hi; v++) set.add(v);
        }
        close_case(&set);
        if (negate)
            for (int k = 0; k < 32; k++) set.bits[k] = (uint8_t)~set.bits[k];
        return leaf(set);
    }

    // ---- grammar ----
    static bool quantifier_start(int c) { return c == '*' || c == '+' || c == '?' || c == '{'; }
    int alt(int depth) {
        int left = concat(depth);
        while (at_ < m_ && p_[at_] == '|') {
            // an empty branch is neither an atom nor a group, yet every '|' is a node that count / min_len / build descend
            if (++atoms_ > MAX_ATOMS) return fail(at_, "too many atoms and branches in the pattern", REGEX_LIMIT);
            at_++;
            const int right = concat(depth);
            left = pair(Node::ALT, left, right);
        }
        return left;
    }
    int concat(int depth) {
        int node = empty();
        while (at_ < m_ && p_[at_] != '|' && p_[at_] != ')') node = cat(node, repeated(depth));
        return node;
    }
    int repeated(int depth) {
        if (quantifier_start(p_[at_])) return fail(at_, p_[at_] == '{' ? "a '{' that is not behind an atom" : "nothing to repeat");
        if (++atoms_ > MAX_ATOMS) return fail(at_, "too many atoms in the pattern", REGEX_LIMIT);
        int node = atom(depth);
        if (status != REGEX_OK || at_ >= m_ || !quantifier_start(p_[at_])) return node;
        const size_t q = at_;
        const int c = p_[at_++];
        uint32_t lo = c == '+' ? 1 : 0, hi = c == '?' ? 1 : INF;
        if (c == '{') {
            auto number = [&](uint32_t *v) {
                const size_t from = at_;
                uint64_t x = 0;
                while (at_ < m_ && is_digit(p_[at_])) x = std::min<uint64_t>(10 * x + (p_[at_++] - '0'), REPEAT_CAP);
                *v = (uint32_t)x;
                return at_ > from;
            };
            if (!number(&lo)) return fail(q, "a '{' that is not {m}, {m,} or {m,n}");
            hi = lo;
            if (at_ < m_ && p_[at_] == ',') {
                at_++;
                if (!number(&hi)) hi = INF;
            }
            if (at_ >= m_ || p_[at_] != '}') return fail(q, "a '{' that is not {m}, {m,} or {m,n}");
            at_++;
            if (hi < lo) return fail(q, "a reversed {m,n}");
        }
        if (at_ < m_ && quantifier_start(p_[at_])) return fail(at_, "lazy, possessive and stacked quantifiers are not supported");
        return repeat(node, lo, hi);
    }
    int atom(int depth) {
        const size_t start = at_;
        const int c = p_[at_++];
        switch (c) {
            case 0: return fail(start, "a NUL byte in the pattern");
            case '^': case '$': return fail(start, "anchors are not supported");
            case '.': return leaf(shorthand('.'));
            case '[': return char_class();
            case '(': {
                if (depth >= MAX_DEPTH) return fail(start, "groups nested too deep", REGEX_LIMIT);
                if (at_ < m_ && p_[at_] == '?') {
                    if (at_ + 1 >= m_ || p_[at_ + 1] != ':')
                        return fail(start, "look-around, inline flags, named and other (?...) groups are not supported");
                    at_ += 2;
                }
                const int inner = alt(depth + 1);
                if (status != REGEX_OK) return inner;
                if (at_ >= m_) return fail(start, "unbalanced '('");
                at_++;                         // alt() stops at the end or at a ')' only
                return inner;                  // one node: a quantifier behind it repeats the whole group
            }
            case '\\': {
                RegexClass set;
                const int b = escape(false, &set);
                if (b == -1) return empty();
                if (b == -2) return leaf(set);
                return literal(b);
            }
            default: return literal(c);
        }
    }
    int literal(int b) {
        RegexClass set;
        set.add(b);
        close_case(&set);
        return leaf(set);
    }
};

}  // namespace

RegexStatus regex_compile(const char *pat, size_t m, bool ignore_case, bool search, RegexProgram *out, size_t *err_offset,
                          const char **err_msg) {
    Compiler c(pat, m, ignore_case);
    int root = c.parse();
    if (c.status == REGEX_OK) {
        if (search) root = c.wrap_search(root);
        if (c.count(root) > REGEX_MAX_POSITIONS) {
            c.status = REGEX_LIMIT;
            c.err_offset = 0;
            c.err_msg = "more pattern positions than FHS_REGEX_MAX_POSITIONS after the counted repeats are expanded";
        }
    }
    if (err_offset) *err_offset = c.status == REGEX_SYNTAX ? c.err_offset : 0;
    if (err_msg) *err_msg = c.err_msg;
    if (c.status != REGEX_OK) return c.status;
    RegexProgram g;
    const Frag f = c.build(root, &g);
    g.first = f.first;
    g.last = f.last;
    g.nullable = f.nullable;
    g.min_len = (size_t)c.min_len(root);
    g.pred.assign(g.positions(), 0);
    for (size_t p = 0; p < g.positions(); p++)
        for (size_t q = 0; q < g.positions(); q++)
            if ((g.follow[p] >> q) & 1) g.pred[q] |= (uint64_t)1 << p;
    *out = g;
    return REGEX_OK;
}

RegexProgram regex_reverse(const RegexProgram &g) {
    RegexProgram r = g;
    std::swap(r.first, r.last);
    r.follow.swap(r.pred);
    return r;
}

}  // namespace fhs
