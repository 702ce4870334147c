// Test probe for the arithmetic of secp256k1_device.hpp: one op selector over packed limb records,
// compiled for the host (_core.secp32_probe, csrc/bind/bind_script.cpp) and for gfx950
// (secp256k1_probe.hip), so both dispatch through this text and tests/test_secp_edges.py can hold
// each primitive against Python integers on either side. Nothing on the verify path uses it.
#pragma once

#include "secp256k1_device.hpp"

// A record is SECP_PROBE_IN_WORDS little-endian limbs in (up to five field elements, unused ones
// ignored) and SECP_PROBE_OUT_WORDS out: three field elements, then one flag word.
#define SECP_PROBE_IN_WORDS 40
#define SECP_PROBE_OUT_WORDS 25

#define SECP_PROBE_F_MUL 0u         // out0 = in0 * in1 mod p (inputs need not be reduced)
#define SECP_PROBE_F_SQR 1u         // out0 = in0^2 mod p
#define SECP_PROBE_F_ADD 2u         // out0 = in0 + in1 mod p, inputs < p
#define SECP_PROBE_F_SUB 3u         // out0 = in0 - in1 mod p, inputs < p
#define SECP_PROBE_F_INV 4u         // out0 = in0^-1 mod p
#define SECP_PROBE_F_SQRT 5u        // flag = in0 is a square, out0 = in0^((p+1)/4)
#define SECP_PROBE_S_MUL 6u         // out0 = in0 * in1 mod n (inputs need not be reduced)
#define SECP_PROBE_S_INV 7u         // out0 = in0^-1 mod n
#define SECP_PROBE_F_GEQ_P 8u       // flag = in0 >= p
#define SECP_PROBE_S_GEQ_N 9u       // flag = in0 >= n
#define SECP_PROBE_S_SUB_N 10u      // out0 = in0 + (2^256 - n) mod 2^256
#define SECP_PROBE_J_DOUBLE 11u     // out0..2 = 2 * (in0, in1, in2) Jacobian
#define SECP_PROBE_J_ADD_AFFINE 12u // out0..2 = (in0, in1, in2) + affine (in3, in4), flag = degenerate
#define SECP_PROBE_NUM_OPS 13u

struct SecpProbeParams {
    const uint32_t* in;  // n x SECP_PROBE_IN_WORDS
    uint32_t* out;       // n x SECP_PROBE_OUT_WORDS
    uint32_t op;
    uint32_t n;
};

namespace secp32 {

SECP_HD F probe_load(const uint32_t* in, int k) {
    F r;
    for (int i = 0; i < 8; ++i) r.v[i] = in[k * 8 + i];
    return r;
}

// One record. Every output word is written (zero where the op leaves it unused); an unknown op
// writes zeros.
SECP_HD void probe_record(uint32_t op, const uint32_t* in, uint32_t* out) {
    const F a = probe_load(in, 0), b = probe_load(in, 1);
    F o[3] = {f_zero(), f_zero(), f_zero()};
    uint32_t flag = 0;
    switch (op) {
        case SECP_PROBE_F_MUL: o[0] = f_mul(a, b); break;
        case SECP_PROBE_F_SQR: o[0] = f_sqr(a); break;
        case SECP_PROBE_F_ADD: o[0] = f_add(a, b); break;
        case SECP_PROBE_F_SUB: o[0] = f_sub(a, b); break;
        case SECP_PROBE_F_INV: o[0] = f_inv(a); break;
        case SECP_PROBE_F_SQRT: flag = f_sqrt(a, o[0]) ? 1u : 0u; break;
        case SECP_PROBE_S_MUL: o[0] = s_mul(a, b); break;
        case SECP_PROBE_S_INV: o[0] = s_inv(a); break;
        case SECP_PROBE_F_GEQ_P: flag = f_geq_p(a) ? 1u : 0u; break;
        case SECP_PROBE_S_GEQ_N: flag = s_geq_n(a) ? 1u : 0u; break;
        case SECP_PROBE_S_SUB_N:
            o[0] = a;
            s_sub_n(o[0]);
            break;
        case SECP_PROBE_J_DOUBLE:
        case SECP_PROBE_J_ADD_AFFINE: {
            J p;
            p.x = a;
            p.y = b;
            p.z = probe_load(in, 2);
            J r;
            if (op == SECP_PROBE_J_DOUBLE) {
                r = j_double(p);
            } else {
                A q;
                q.x = probe_load(in, 3);
                q.y = probe_load(in, 4);
                bool deg = false;
                r = j_add_affine(p, q, deg);
                flag = deg ? 1u : 0u;
            }
            o[0] = r.x;
            o[1] = r.y;
            o[2] = r.z;
            break;
        }
        default: break;
    }
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 8; ++i) out[k * 8 + i] = o[k].v[i];
    out[24] = flag;
}

}  // namespace secp32
