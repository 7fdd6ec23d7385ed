// verify_half_item_body.h — the per-item body of the fixed-generator verify equation, as TEXT: the statements that
// k_verify_fixed_half (k_verify.hip, where the method is described) and listed_item_ok (k_keyed_open.hip) both run.
// A fragment, not a function — no include guard, no namespace: it is #included inside a scope that provides
//   bool good                 the item's verdict so far, narrowed here
//   size_t i                  the item's row (scalars u, c)
//   const uint8_t *u, *c      the scalar columns
//   ChainOperands op0, op1    the operands of chain 0 / chain 1
//   JointTable tbl            the lane's window table
//   int NCHAIN                the number of chains (1 or 2)
// and the two macros, defined immediately before the #include and #undef'd immediately after it:
//   DSV_ITEM_ROW_SETUP        statements in front of the four point loads of a chain (may be empty)
//   DSV_ITEM_ROW              the row those loads address (2 * ROW, 2 * ROW + 1)
// Text, because the body moved into a function or a function template that both kernels call gives
// k_verify_fixed_half another register allocation; included as text, both kernels compile to the
// instructions they had as two copies.
u32 ya[8], yb[8], w[8];
bool b_neg;
int top;
{
  u32 cs[8], a[8], b[8];
  load_words8(cs, c, i);
  half_scalars(a, b, b_neg, cs);
  // signed 2-bit digits of a and |b| (the sign of the R term goes into the point: -R below)
  recode_signed2(ya, a);
  recode_signed2(yb, b);
  u32 nz[8];
#pragma unroll
  for (int k = 0; k < 8; k++) nz[k] = (ya[k] ^ 0x55555555u) | (yb[k] ^ 0x55555555u);
  top = top_digit2(nz);
  u32 us[8];
  load_words8(us, u, i);
  const bool u_ok = words_lt(us, kR32);
  good &= u_ok;
  if (!u_ok) us[7] &= 0x0fffffffu;  // keep fr_mul's inputs below r-ish; verdict is 0 anyway
  fr_mul(w, b, us);                 // |b| * u mod r
  if (b_neg) {                      // (b*u) mod r with b < 0
    const u32 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    u32 t[8];
    fr_sub(t, zero, w);
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = t[k];
  }
}
#pragma unroll 1
for (int h = 0; h < NCHAIN; h++) {
  const ChainOperands op = h ? op1 : op0;
  {
    DSV_ITEM_ROW_SETUP
    Fe pku, pkv, ru, rv;
    good &= load_fq(pku, op.PK_uv, 2 * DSV_ITEM_ROW);
    good &= load_fq(pkv, op.PK_uv, 2 * DSV_ITEM_ROW + 1);
    good &= load_fq_signed(ru, op.R_uv, 2 * DSV_ITEM_ROW, !b_neg);  // the chain adds -|b| * R unless b < 0
    good &= load_fq(rv, op.R_uv, 2 * DSV_ITEM_ROW + 1);
    build_joint_table(tbl, pku, pkv, ru, rv);
  }
  // T = a*PK + |b|*(-+R) (+ w*G below): one joint entry per 2-bit window, loaded one window ahead
  Ext acc = ext_from_niels(load_joint_entry(tbl, joint_digit(ya, yb, top)));
  {
    RawJoint e = load_joint_entry_raw(tbl, joint_digit(ya, yb, top > 0 ? top - 1 : 0));
#pragma unroll 1
    for (int k = top - 1; k >= 0; k--) {
      acc = ext_mul4(acc);
      const Niels cur = finish_joint_entry(e);
      e = load_joint_entry_raw(tbl, joint_digit(ya, yb, k > 0 ? k - 1 : 0));  // last: unused
      acc = ext_add_niels(acc, cur);
    }
  }
  // T + w*G == O  (T == O  <=>  u == 0 and v == z, decided inside the last addition)
  good &= fixed_base_accumulate_is_identity(acc, w, op.table);
}
