// Regular expressions against a CLEAR pattern: the host-only half.  A strict subset of Python's
// bytes `re` syntax is parsed and compiled into its position (Glushkov) automaton; Strings::regex evaluates that
// automaton on encrypted characters.  Nothing here touches an engine.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fhs {

constexpr size_t REGEX_MAX_POSITIONS = 64;   // FHS_REGEX_MAX_POSITIONS: a set of positions is one 64-bit word

struct RegexClass {                           // a set of bytes, NUL never among them
    uint8_t bits[32] = {0};
    bool has(int v) const { return (bits[v >> 3] >> (v & 7)) & 1; }
    void add(int v) { bits[v >> 3] |= (uint8_t)(1u << (v & 7)); }
    int count() const;
    bool operator==(const RegexClass &o) const;
};

// The automaton of a pattern: positions 0 .. P-1 (the paper's 1 .. P), each reading one class.  Every edge into q reads
// q's class, so follow / pred are plain sets of positions.
struct RegexProgram {
    std::vector<RegexClass> classes;          // distinct classes
    std::vector<int> cls;                     // per position: index into classes
    std::vector<uint64_t> follow, pred;       // per position
    uint64_t first = 0, last = 0;
    bool nullable = false;
    size_t min_len = 0;                       // length of the shortest match
    size_t positions() const { return cls.size(); }
    bool matches_everything() const;          // sufficient, not necessary: nullable, and one position that reads any
                                              // character, starts, loops on itself and ends (`.*`, SEARCH of a nullable)
};

enum RegexStatus { REGEX_OK = 0, REGEX_SYNTAX, REGEX_LIMIT };
// pat[m] -> program.  ignore_case closes every positive set under the case swap of ASCII letters (a negated class is
// the complement of the closed set); search compiles .*(?:pat).* -- its two positions count.  REGEX_SYNTAX: *err_offset
// is the byte offset of the first byte of what is refused.  REGEX_LIMIT: more than
// REGEX_MAX_POSITIONS positions after the counted repeats are expanded ({m,n}: n copies; {m,}: max(m, 1) copies).
RegexStatus regex_compile(const char *pat, size_t m, bool ignore_case, bool search, RegexProgram *out, size_t *err_offset,
                          const char **err_msg);

// The automaton of the reversed language: first and last change places, and so do follow and
// pred; classes, the nullable bit and min_len stay.  Run from the right end of a text it says where a match STARTS.
RegexProgram regex_reverse(const RegexProgram &g);

}  // namespace fhs
