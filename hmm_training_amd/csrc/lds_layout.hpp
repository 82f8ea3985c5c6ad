// lds_layout.hpp — geometry of the small kernels' LDS emission tables (hmmbw_device.hpp): the row layout's
// table distance and sizes, and the address functions of the class-split layout (LAY = 1).
// Plain constexpr C++ with no HIP dependency, so that a host compiler can build a probe of them
// (tests/native/lds_layout_probe.cpp).
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define HMMBW_HD __host__ __device__
#else
#define HMMBW_HD
#endif

namespace hmmbw {

// The row layout (LAY = 0): two [K][G] tables of 16-B entries, the H-table kHistOff bytes after the P-table.
// The kernels use them when the P-table fits below kHistOff (the row offsets then fit the uint16 symbol packs).
constexpr int kHistOff = 32768;
HMMBW_HD constexpr bool lds_tables_fit(int K, int GP) { return (size_t)K * GP * 16 <= (size_t)kHistOff; }
HMMBW_HD constexpr size_t lds_table_bytes(int K, int GP) { return (size_t)kHistOff + (size_t)K * GP * 16; }

// The class-split layout (LAY = 1) of the joined map's G = 8 kernels (k_estep_join<.., 1>), which own a whole
// CU's LDS.  In the row layout (hmmbw_device.hpp) a ds_read_b128 lane group ({0-3, 12-15, 20-27}, ... MI355X: four 16-B windows
// of four states, of sequence slots 0, 1, 2, 3) puts slots 0 and 3 (states 0-3) and slots 1 and 2 (states 4-7)
// on the same 16 banks whenever their symbols have equal parity: 1.74 LDS cycles per group on uniform symbols
// (tools/lds_banks.py).  Here slot u reads the tables of its class (u >> 1) & 1, and each class owns K rows of
//   [ P row: GP x {x, y} | H row: GP x {h_even, h_odd} ]   (2 GP 16 bytes, 256 for G = 8; halves: lay2_add_off)
// with class 1's region 65,536 + GP 16 bytes after class 0's, so class 0's P rows lie on banks 0-31 of the
// read's 64 and class 1's on banks 32-63: the four windows of a lane group fall on four different bank
// quarters whatever the symbols (1.00 cycles per group).  The packs hold o 2 GP 16 (<= 65,280 at K = 256:
// uint16 still), the lane's base adds the class offset once per wave, and H - P is the constant GP 16, the
// immediate offset of the histogram add.  Both classes hold the same P; each accumulates its own slots'
// histogram, summed at the flush.
HMMBW_HD constexpr int lay2_row_bytes(int GP) { return 2 * GP * 16; }
HMMBW_HD constexpr int lay2_hist_off(int GP) { return GP * 16; }  // H entry - P entry
HMMBW_HD constexpr int lay2_class_off(int GP) { return 65536 + GP * 16; }
// class of sequence slot u: slots 0|3 and 1|2 of a read group apart; the two slots 2i, 2i + 1 of a ds_add_f64 lane
// group together, so their adds meet as in layout 0 (u & 1 would cost skewed symbols a second add cycle in the model)
HMMBW_HD constexpr int lay2_class(int u) { return (u >> 1) & 1; }
HMMBW_HD constexpr bool lay2_tables_fit(int K, int GP) { return (size_t)K * lay2_row_bytes(GP) <= 65536; }
HMMBW_HD constexpr size_t lay2_table_bytes(int K, int GP) {
    return (size_t)lay2_class_off(GP) + (size_t)K * lay2_row_bytes(GP);
}
// byte offset of the P entry of (class, symbol o, state column j); the pack entry of symbol o is lay2_p_off(GP, 0, o, 0)
HMMBW_HD constexpr size_t lay2_p_off(int GP, int cls, int o, int j) {
    return (size_t)cls * lay2_class_off(GP) + (size_t)o * lay2_row_bytes(GP) + (size_t)j * 16;
}

// Parity halves of the histogram.  A ds_add_f64 serves 16 contiguous lanes = the sequence slots 2i, 2i + 1, which
// share a class; with H entries {h, b} both slots' eight h fields lie on the same 16 of the add's 32 banks
// (2.00 cycles per group on uniform symbols, tools/lds_banks.py).  The H entry of the class-split layout is
// therefore {h_even, h_odd}: slot u adds into half u & 1, the two slots of an add group use disjoint bank pairs
// whatever their symbols (1.00), and the flush sums the four pieces (2 classes x 2 halves) of (symbol, state).
// The add's lane address is the read's + lay2_add_off, formed beside it one chunk ahead (the read must stay
// 16-B aligned, so the 8 cannot ride in the shared address).
HMMBW_HD constexpr int lay2_add_off(int GP, int u) { return lay2_hist_off(GP) + 8 * (u & 1); }
// b_j(o) itself, which the left-to-right forward needs once per sweep (pi_j b_j(o_0)), lives in a compact
// [K][GP] fp64 table after the class tables; its rows are a quarter of a P/H row, so a pack entry
// (o lay2_row_bytes) >> kLay2BPackShift is the symbol's row offset in it.
HMMBW_HD constexpr size_t lay2_b_off(int K, int GP, int o, int j) {
    return lay2_table_bytes(K, GP) + ((size_t)o * GP + (size_t)j) * 8;
}
constexpr int kLay2BPackShift = 2;
static_assert(lay2_row_bytes(8) >> kLay2BPackShift == 8 * 8 && lay2_row_bytes(3) >> kLay2BPackShift == 3 * 8, "b row = P/H row / 4");
HMMBW_HD constexpr size_t lay2_b_bytes(int K, int GP) { return (size_t)K * GP * 8; }
// dynamic LDS of the layout ahead of the reduction scratch: class tables + b table
HMMBW_HD constexpr size_t lay2_total_bytes(int K, int GP) { return lay2_table_bytes(K, GP) + lay2_b_bytes(K, GP); }
// a CU's LDS (one workgroup per CU owns it all) and what the joined kernel needs beside the tables: the
// reduction scratch (dynamic; at most [8 waves][8][N + 3] + 16 doubles, N = 8) and its static LDS (M-step
// scratch, parameters, hand-over slots: under 4 KiB in every instantiation)
constexpr size_t kCuLdsBytes = 160 * 1024;
constexpr size_t kLay2OtherBytes = 8 * (8 * 8 * 11 + 16) + 4096;
HMMBW_HD constexpr bool lay2_lds_fit(int K, int GP, size_t other = kLay2OtherBytes) {
    return lay2_tables_fit(K, GP) && lay2_total_bytes(K, GP) + other <= kCuLdsBytes;
}
static_assert(lay2_total_bytes(256, 8) == 147584 && lay2_lds_fit(256, 8) && !lay2_lds_fit(257, 8), "K = 256 fits a CU");

}  // namespace hmmbw
