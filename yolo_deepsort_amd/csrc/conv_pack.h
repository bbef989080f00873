// Weight rows of the implicit-GEMM convolutions, packed on the host.  Plain C++: no device call, no device header.
//
// A filter is one row of kpad floats: k index = (kh * ksize + kw) * cin + c (cin = the channel-padded input the kernel reads),
// zero padded to kpad, a multiple of 32.
#pragma once
#include <stddef.h>
#include <string.h>
#include <vector>

namespace yds {

inline int conv_kpad(int ksize, int cin) { return (ksize * ksize * cin + 31) / 32 * 32; }

// OIHW w[cout][cin_file][ksize][ksize] -> rows[cout][kpad]; scale (optional): one double per filter (folded BatchNorm), the product
// is taken in double and rounded once
inline void pack_conv_rows(const float *w, int cout, int cin_file, int cin, int ksize, const double *scale, std::vector<float> &rows) {
    const int kpad = conv_kpad(ksize, cin);
    rows.assign((size_t)cout * kpad, 0.f);
    for (int o = 0; o < cout; ++o)
        for (int c = 0; c < cin_file; ++c)
            for (int kh = 0; kh < ksize; ++kh)
                for (int kw = 0; kw < ksize; ++kw)
                    rows[(size_t)o * kpad + (kh * ksize + kw) * cin + c] =
                        (float)((double)w[(((size_t)o * cin_file + c) * ksize + kh) * ksize + kw] * (scale ? scale[o] : 1.0));
}

// the same from weights already in k order, w[cout][ksize * ksize * cin]: only the row padding is added
inline void pack_conv_rows_korder(const float *w, int cout, int cin, int ksize, std::vector<float> &rows) {
    const int K = ksize * ksize * cin, kpad = conv_kpad(ksize, cin);
    rows.assign((size_t)cout * kpad, 0.f);
    for (int o = 0; o < cout; ++o) memcpy(&rows[(size_t)o * kpad], w + (size_t)o * K, (size_t)K * sizeof(float));
}

}  // namespace yds
