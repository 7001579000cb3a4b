// word_stream.h -- the wire format of the CPU model programs (tools/*_check.cpp), stated once: stdin and stdout are
// streams of little-endian int64 words; a float64 travels as its bits, a float32 as its bits in the low half of a word.
// A program reads with read_word / read_ints / read_doubles / read_floats, appends what it has to say to `out`, and
// ends with `return flush();` -- one fwrite of everything, so a program that stops on an error writes nothing.
// tests/model_harness.py is the Python half.  Included with quotes: every tool stays a one-file program that the g++ line
// in its header comment builds.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

namespace word_stream {

// n elements as they lie in the stream; words, or the packed payload a tool's own format carries (topk_model_check's rows)
template <class X> bool read_raw(X *dst, size_t n) { return fread(dst, sizeof(X), n, stdin) == n; }
inline bool read_words(int64_t *dst, size_t n) { return read_raw(dst, n); }
// the next word, 0 once the input has ended; *ok stays false from then on
inline int64_t read_word(bool *ok) { int64_t v = 0; *ok = *ok && read_words(&v, 1); return v; }
inline double as_double(int64_t bits) { double d; memcpy(&d, &bits, 8); return d; }
inline float as_float(int64_t bits) { const uint32_t b = (uint32_t)bits; float f; memcpy(&f, &b, 4); return f; }
inline int64_t as_bits(double d) { int64_t b; memcpy(&b, &d, 8); return b; }
inline int64_t as_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return (int64_t)b; }  // zero-extended

// dst.size() words, each converted to the element type of dst
template <class V> bool read_ints(V &dst) {
    std::vector<int64_t> w(dst.size());
    if (!read_words(w.data(), w.size())) return false;
    for (size_t i = 0; i < w.size(); i++) dst[i] = (typename V::value_type)w[i];
    return true;
}
inline bool read_doubles(std::vector<double> &dst) {
    std::vector<int64_t> w(dst.size());
    if (!read_words(w.data(), w.size())) return false;
    for (size_t i = 0; i < w.size(); i++) dst[i] = as_double(w[i]);
    return true;
}
inline bool read_floats(std::vector<float> &dst) {
    std::vector<int64_t> w(dst.size());
    if (!read_words(w.data(), w.size())) return false;
    for (size_t i = 0; i < w.size(); i++) dst[i] = as_float(w[i]);
    return true;
}

inline std::vector<int64_t> out;
template <class V> void put(const V &v) { for (auto x : v) out.push_back((int64_t)x); }
template <class F> void put_bits(const std::vector<F> &v) { for (F x : v) out.push_back(as_bits(x)); }
// what main returns when all went well
inline int flush() {
    if (fwrite(out.data(), sizeof(int64_t), out.size(), stdout) != out.size()) { fprintf(stderr, "short write\n"); return 2; }
    return 0;
}

}  // namespace word_stream
