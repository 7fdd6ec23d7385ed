// verify_var_item_body.h — the per-item body of the var-generator verify equation, as TEXT: the statements that
// k_verify_var (k_vargen.hip, where the method is described) and k_verify_var_listed (k_keyed_open_var.hip) both
// run.  A fragment, not a function — no include guard, no namespace: it is #included inside a scope that provides
//   bool good                           the item's verdict so far, narrowed here
//   size_t i                            the item's row, in every column
//   const uint8_t *u, *c                the scalar columns
//   const uint8_t *Gen_uv, *PK_uv, *R_uv  the point columns
//   u32 *tg, *tp, *tr                   the lane's three window tables (Gen, PK, R)
// Text for the reason verify_half_item_body.h is: both kernels compile to the instructions they
// had as two copies.
u32 yx[8], yy[8], yz[8];
int sx, sy, sz, top;
{
  u32 us[8], cs[8], mx[8], my[8], mz[8];
  bool nx, ny, nz;
  load_words8(us, u, i);
  load_words8(cs, c, i);
  good &= words_lt(us, kR32);
  if (!words_lt(us, kR32)) us[7] &= 0x0fffffffu;  // keep the scalars in range; verdict is 0 anyway
  lattice3_scalars(mx, my, mz, nx, ny, nz, us, cs);
  recode_signed4(yx, mx);
  recode_signed4(yy, my);
  recode_signed4(yz, mz);
  u32 nzd[8];
#pragma unroll
  for (int k = 0; k < 8; k++)
    nzd[k] = (yx[k] ^ 0x88888888u) | (yy[k] ^ 0x88888888u) | (yz[k] ^ 0x88888888u);
  top = top_digit4(nzd);
  sx = nx ? -1 : 1;
  sy = ny ? -1 : 1;
  sz = nz ? 1 : -1;  // the chain adds (-z) * R
}
{
  Fe gu, gv;
  good &= load_fq(gu, Gen_uv, 2 * i);
  good &= load_fq(gv, Gen_uv, 2 * i + 1);
  build_var_table(tg, gu, gv);
}
{
  Fe pku, pkv;
  good &= load_fq(pku, PK_uv, 2 * i);
  good &= load_fq(pkv, PK_uv, 2 * i + 1);
  build_var_table(tp, pku, pkv);
}
{
  Fe ru, rv;
  good &= load_fq(ru, R_uv, 2 * i);
  good &= load_fq(rv, R_uv, 2 * i + 1);
  build_var_table(tr, ru, rv);
}
Ext acc = ext_from_niels(load_var_entry(tg, sx * sdigit4(yx, top)));
acc = ext_add_niels(acc, load_var_entry(tp, sy * sdigit4(yy, top)));
acc = ext_add_niels(acc, load_var_entry(tr, sz * sdigit4(yz, top)));
{
  const int k0 = top > 0 ? top - 1 : 0;
  RawNiels ea = load_var_entry_raw(tg, sx * sdigit4(yx, k0));
#pragma unroll 1
  for (int k = top - 1; k >= 0; k--) {
    acc = ext_mul16(acc);
    const RawNiels eb = load_var_entry_raw(tp, sy * sdigit4(yy, k));
    acc = ext_add_niels(acc, finish_var_entry(ea));
    const RawNiels ec = load_var_entry_raw(tr, sz * sdigit4(yz, k));
    acc = ext_add_niels(acc, finish_var_entry(eb));
    const int kn = k > 0 ? k - 1 : 0;  // last round: reloads its own entry, unused
    ea = load_var_entry_raw(tg, sx * sdigit4(yx, kn));
    acc = ext_add_niels(acc, finish_var_entry(ec));
  }
}
// T == O  <=>  u == 0 and v == z
good &= (bool)((int)fe_is_zero_canon(fe_canon(acc.u)) & (int)fe_equal(acc.v, acc.z));
