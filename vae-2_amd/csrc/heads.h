// What crosses heads.hip, upadj.hip and resample.hip (internal to libvae2_hip.so).
#pragma once

#include "common.h"

namespace vae2 {

constexpr int kUsXB = 64;  // output pixels per chunk of a row: up-sum forward and adjoints
constexpr int kAdjBandDefault = 32;  // g_adj_band: dy rows per one-pass adjoint workgroup
// vae2_heads_set_algo switches (kSwitches, heads.hip, documents each), defined where read.
extern int g_adj_stream, g_adj_fused, g_adj_band, g_fuse_adj3;  // upadj.hip
extern int g_relu_dual_q;                                        // resample.hip

}  // namespace vae2
