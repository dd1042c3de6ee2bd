// bicg_spmv_sell_lay.hip -- the instantiations of ONE sliced-ELL layout (96 SpMV kernels + 12 with an epilogue). The Makefile
// compiles this file once per layout of SELL_LAYS with -DBICG_SELL_LAY=LAY_<name>: a few hundred kernels each, built in parallel,
// one code object each.
#include "bicg_spmv_sell.h"

#ifndef BICG_SELL_LAY
#error "compile with -DBICG_SELL_LAY=<one SellLayout>"
#endif

namespace bicg {

template bool sell_launch_layout<BICG_SELL_LAY>(SELL_LAY_ARGS);
template bool sell_epi_launch_layout<BICG_SELL_LAY>(SELL_LAY_ARGS);
template void preload_layout<BICG_SELL_LAY>();

}  // namespace bicg
