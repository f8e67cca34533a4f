// The dual-use image of the high fp16 plane of a 32-key x 128-channel tile of f ("kv_fold" with the fp8 attention body, DESIGN
// section 3): ONE 8 KiB image serves S = K Q'^T, which reads it by rows (ds_read_b128: a key's 8 channels of a k-step), and
// O^T += V^T P^T, which reads it by columns (ds_read_b64_tr_b16: a feature's 4 consecutive keys).  Free of HIP: the linear kernel
// writes through it, the attention kernel reads through it, tests/abi_cpp/kv_share_layout_host.cpp holds both reads to the two
// fragment-major images they replace, lane for lane, and counts their bank conflicts.
//
// A row is a key; its 16 chunks of 16 bytes hold the channels in FRAGMENT order: chunk 2 s + h = the 8 values a lane of half h holds
// for k-step s (register e of them = channel 16 s + 8 (e >> 2) + 4 h + (e & 3), frag_feature in mfma_core.hpp).  So the four values
// at byte 8 a of chunk 2 s + h are the CONSECUTIVE channels 16 s + 8 a + 4 h .. + 3 - what a transposed read hands to four
// neighbouring lanes.  The rows lie in 8-row x 4-chunk subtiles of 512 bytes with the chunk index XORed by (row >> 2) & 3: both
// kinds of read touch every bank once, and the addresses of one kind differ between lanes in only two ways (2 + 2 address
// registers; everything else is an immediate offset).
#pragma once

namespace gmf {
namespace kvshare {

constexpr unsigned kPlaneBytes = 32 * 128 * 2;

// byte offset of chunk `ch` (0..15) of key `row` (0..31)
constexpr unsigned off(unsigned row, unsigned ch) {
  return 2048u * (row >> 3) + 512u * (ch >> 2) + 64u * (row & 7u) + 16u * ((ch & 3u) ^ ((row >> 2) & 3u));
}

// Row read (the A operand of S, v_mfma_f32_32x32x16_f16): lane (h = lane >> 5, key i = lane & 31) reads the 16 bytes of k-step s.
// = row_read_addr(lane, s & 1) + 512 (s >> 1)
constexpr unsigned row_read_addr(unsigned lane, unsigned s) { return off(lane & 31u, 2u * s + (lane >> 5)); }

// Transposed read (the A operand of O^T: the lane's feature, 4 consecutive keys): the address lane `lane` SUPPLIES for feature block
// db (features 32 db ..) and key group kg (keys 4 kg .. 4 kg + 3).  Lane 4 q + p of a 16-lane group g supplies key 4 kg + q and the
// four values that lanes 4 p .. 4 p + 3 of the group receive: features 32 db + 16 (g & 1) + 4 p .. + 3.
// The operand of k-step s2 is two such reads, kg = 4 s2 + (lane >> 5) and that + 2 (frag_feature's two groups of four keys).
// = tr_read_addr(lane, 0, kg & 3) + 512 db + 4096 (kg >> 2)
constexpr unsigned tr_read_addr(unsigned lane, unsigned db, unsigned kg) {
  const unsigned j = lane & 15u, q = j >> 2, p = j & 3u, gb = (lane >> 4) & 1u;
  return off(4u * kg + q, 4u * db + 2u * gb + (p & 1u)) + 8u * (p >> 1);
}

}  // namespace kvshare
}  // namespace gmf
