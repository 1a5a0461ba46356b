// The embed kernels' key decision (thatsmyface_amd/csrc/tmfwm_embed_key.h) compiled for the
// host: tests/test_embed_key.py calls it through ctypes.
#include "../../thatsmyface_amd/csrc/tmfwm_embed_key.h"

extern "C" {

// embed_key_decide on the two ends
int ek_decide(float tl, float th, float *key)
{
    const tmf::KeyDecision d = tmf::embed_key_decide(tl, th);
    *key = d.key;
    return d.decided ? 1 : 0;
}

// embed_key_of over n (sigma, tE) pairs
void ek_of(const double *sigma, const double *tE, long long n, unsigned char *decided, float *key)
{
    for (long long i = 0; i < n; ++i) {
        const tmf::KeyDecision d = tmf::embed_key_of(sigma[i], tE[i]);
        decided[i] = d.decided ? 1 : 0;
        key[i] = d.key;
    }
}

int ek_fused(int block)
{
    switch (block) {
    case 4: return tmf::kEmbedKeyFused<4>;
    case 6: return tmf::kEmbedKeyFused<6>;
    case 8: return tmf::kEmbedKeyFused<8>;
    case 10: return tmf::kEmbedKeyFused<10>;
    case 12: return tmf::kEmbedKeyFused<12>;
    case 14: return tmf::kEmbedKeyFused<14>;
    case 16: return tmf::kEmbedKeyFused<16>;
    default: return -1;
    }
}

}  // extern "C"
