#include "conv_weights.h"

namespace yds {

void ConvWeights::upload_rows(const std::vector<float> &rows, const float *bias_host, hipStream_t s) {
    std::vector<uint16_t> split;
    pack_weights_f16x3(rows.data(), cout, kpad, split);
    wt.upload(rows.data(), rows.size(), s);
    wt16.upload(split.data(), split.size(), s);
    bias.upload(bias_host, (size_t)cout, s);
    YDS_HIP(hipStreamSynchronize(s));                           // rows and split go away
}

void ConvWeights::upload(const float *oihw, const double *scale, const float *bias_host, hipStream_t s) {
    std::vector<float> rows;
    pack_conv_rows(oihw, cout, cin_file, cin, ksize, scale, rows);
    upload_rows(rows, bias_host, s);
}

void ConvWeights::upload_korder(const float *w_okkc, const float *bias_host, hipStream_t s) {
    std::vector<float> rows;
    pack_conv_rows_korder(w_okkc, cout, cin, ksize, rows);
    upload_rows(rows, bias_host, s);
}

ConvWeights ConvWeights::concat(const ConvWeights &a, const ConvWeights &b, hipStream_t s) {
    if (a.kpad != b.kpad) fail("conv weights: concatenating filters of %d and %d columns", a.kpad, b.kpad);
    ConvWeights m;
    m.shape(a.cout + b.cout, a.cin_file, a.cin, a.ksize, a.stride, a.pad);
    const size_t na = (size_t)a.cout * a.kpad, nb = (size_t)b.cout * b.kpad;
    m.wt.alloc(na + nb); m.wt16.alloc(2 * (na + nb)); m.bias.alloc((size_t)m.cout);
    auto d2d = [&](void *dst, const void *src, size_t bytes) { YDS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s)); };
    d2d(m.wt.p, a.wt.p, na * 4);                    d2d(m.wt.p + na, b.wt.p, nb * 4);
    d2d(m.wt16.p, a.wt16.p, na * 4);                d2d(m.wt16.p + 2 * na, b.wt16.p, nb * 4);
    d2d(m.bias.p, a.bias.p, (size_t)a.cout * 4);    d2d(m.bias.p + a.cout, b.bias.p, (size_t)b.cout * 4);
    YDS_HIP(hipStreamSynchronize(s));
    return m;
}

}  // namespace yds
