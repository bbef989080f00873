// One convolution's folded weights on the device, in the three forms the kernels take, with the geometry that fixes their layout.
#pragma once
#include "common.h"
#include "conv_pack.h"

namespace yds {

struct ConvWeights {
    int cout = 0, cin = 0, cin_file = 0;     // cin: channel-padded input the kernel reads; cin_file: input channels of the weight file
    int ksize = 1, stride = 1, pad = 0, kpad = 0;
    DevBuf<float> wt, bias;                  // [cout][kpad] rows (conv_pack.h), [cout]
    DevBuf<uint16_t> wt16;                   // the rows pre-split for the f16x3 kernels (pack_weights_f16x3)

    void shape(int cout_, int cin_file_, int cin_, int ksize_, int stride_, int pad_) {
        cout = cout_; cin_file = cin_file_; cin = cin_; ksize = ksize_; stride = stride_; pad = pad_;
        kpad = conv_kpad(ksize, cin);
    }
    bool loaded() const { return wt.p != nullptr; }
    void release() { wt.release(); bias.release(); wt16.release(); }
    // OIHW weights [cout][cin_file][ksize][ksize] (times scale[o] when given), bias_host[cout]; shape() comes first.  Returns after
    // the copies have completed on s.
    void upload(const float *oihw, const double *scale, const float *bias_host, hipStream_t s);
    void upload_korder(const float *w_okkc, const float *bias_host, hipStream_t s);     // weights [cout][ksize * ksize * cin]
    void fill(ConvArgs &a) const {
        a.w = wt.p; a.w16 = wt16.p; a.bias = bias.p;
        a.ksize = ksize; a.stride = stride; a.pad = pad; a.kpad = kpad;
    }
    // [a's filters ; b's filters] of two convolutions of one tensor (same K), copied on the device
    static ConvWeights concat(const ConvWeights &a, const ConvWeights &b, hipStream_t s);

private:
    void upload_rows(const std::vector<float> &rows, const float *bias_host, hipStream_t s);
};

}  // namespace yds
